"""CPU: the output-rate resampler's filter (mio_hip_resampler_create without a device). For every
accepted rate from 44 100 Hz the phase table equals the float64 formula of include/mio_hip.h rounded
to f32, and its float64 response meets the specification: at or below -79 dB from pi / F up, within
+-0.002 dB up to 0.8 pi / F (the formula gives -79.42 dB at worst and +0.001 dB, rounded outwards)."""
import math

import numpy as np
import pytest

import miotts_amd as m

RATES = [8000, 16000, 22050, 24000, 32000, 48000]
TAPS = {8000: 278, 16000: 140, 22050: 102, 24000: 94, 32000: 70, 48000: 52}


def formula(f_in, f_out):
    g = math.gcd(f_in, f_out)
    L, M = f_out // g, f_in // g
    F, A = max(L, M), 80.0
    P = math.ceil(((A - 7.95) / (2.285 * 0.2 * np.pi / F) + 1) / L)
    P += P & 1
    n, wc = np.arange(P * L), 0.9 * np.pi / F
    h = L * (wc / np.pi) * np.sinc(wc * (n - (P * L - 1) / 2) / np.pi) * np.kaiser(P * L, 0.1102 * (A - 8.7))
    return L, M, P, h.astype(np.float32).reshape(P, L).T  # c[phi][j] = h[j L + phi]


@pytest.mark.parametrize("f_out", RATES)
def test_table_is_the_formula_and_meets_the_spec(f_out):
    r = m.Resampler(None, 44100, f_out)
    L, M, P, want = formula(44100, f_out)
    assert (r.L, r.M, r.P, r.delay) == (L, M, P, P // 2) and P == TAPS[f_out]
    assert L * P * 4 <= 128 * 1024 and r.tile % 64 == 0
    c = r.coeffs()
    np.testing.assert_array_equal(c, want)
    h = c.T.reshape(-1).astype(np.float64)  # phases re-interleaved
    H = np.abs(np.fft.rfft(h, 1 << 22)) / L
    w = np.arange(H.size) * (2 * np.pi / (1 << 22))
    F = max(L, M)
    stop = 20 * np.log10(H[w >= np.pi / F].max())
    ripple = np.abs(20 * np.log10(H[w <= 0.8 * np.pi / F])).max()
    print(f"{f_out} Hz: L={L} M={M} P={P} stopband {stop:.2f} dB, passband ripple {ripple:.4f} dB")
    assert stop <= -79.0 and ripple <= 0.002
    for n in (0, 1, M, M + 1, 1_234_800):
        assert r.out_len(n) == math.ceil(n * L / M)


@pytest.mark.parametrize("f_out", [44100, 12000, 11025, 96000, 0])
def test_unlisted_rate_is_refused_by_name(f_out):
    with pytest.raises(m.HipError, match=f"rate {f_out} Hz"):
        m.Resampler(None, 44100, f_out)

