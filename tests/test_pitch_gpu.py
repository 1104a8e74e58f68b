"""GPU: pitch (csrc/hip/pcm_pitch.hip, mio_hip_pcm_pitch) against tests/np_pitch.py, the float64
restatement of include/mio_hip.h "pitch".

With u = 2^-24, T = 2 K taps and S_j = c sum |x| |h|, the kernel's output is off by at most
(T + 4) u S_j + 2^-149: the f32 FMA chain of T terms (T u), and four more roundings for the f32 table
difference, the f32 interpolation of the coefficient, its fraction and the final product by c. The
table position is formed in float64 by the definition's own expression, so kernel and reference
read the same two entries. Each test prints the worst err / bound it measured.

The refusal of a time-scale outside 0.5 .. 2 is tested with speed 2 at -12 semitones (s1 = 4):
speed 2 at +12 gives s1 = speed / r = 1, the very case the kernel tests below run to skip WSOLA."""
import math
import os
import subprocess
import wave

import numpy as np
import pytest

import miotts_amd as m
import np_pitch as ref

pytestmark = pytest.mark.gpu

BIN = os.path.join(m.PKG_ROOT, "build")
TILE = m.PITCH_TILE
X = (0.3 * np.random.default_rng(11).standard_normal(300000) + 0.4 * np.sin(0.05 * np.arange(300000))).astype(np.float32)


def resample_only(device, xs, st):
    """speed == r: s1 = 1, WSOLA is skipped and the call is the new kernel alone."""
    return m.pcm_pitch(device, xs, st, speed=m.pitch_ratio(st))


def check(x, st, y, first=0):
    r = m.pitch_ratio(st)
    want, S = ref.pitch(x, r, first)
    assert y.shape == (math.ceil(len(x) / r),)
    ratio = np.abs(y[first:] - want) / ((2 * ref.taps(r)[1] + 4) * 2.0 ** -24 * S + 2.0 ** -149)
    print(f"{st:+d} semitones, n={len(x)}: worst err / bound = {ratio.max(initial=0.0):.3g}")
    assert (ratio <= 1.0).all()


@pytest.mark.parametrize("size", [1, 37, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@pytest.mark.parametrize("st", [-12, -7, -1, 1, 4, 12])
def test_kernel_against_definition(device, st, size):
    """`size` input samples, and the shortest input that yields at least `size` outputs."""
    for n in (size, math.floor((size - 1) * m.pitch_ratio(st)) + 1):
        check(X[:n], st, resample_only(device, [X[:n]], st)[0])


def test_batch_of_three_lengths(device):
    xs = [X[:0], X[100:137], X[500:501 + 2 * TILE]]
    for x, y in zip(xs, resample_only(device, xs, 4)):
        check(x, 4, y)


def test_no_drift(device):
    """The last 2000 of 283 000 outputs: a position kept in f32, or accumulated, is off by samples here."""
    y = resample_only(device, [X], 1)[0]
    check(X, 1, y, first=y.size - 2000)


@pytest.mark.parametrize("s", [0.8, 1.25])
def test_pitch_zero_is_pcm_speed(device, s):
    y, want = m.pcm_pitch(device, [X[:20000]], 0, s)[0], m.pcm_speed(device, [X[:20000]], s)[0][0]
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))


def test_duration_kept_and_tone_moved(device):
    x = np.sin(2 * np.pi * 220.0 / 44100 * np.arange(88200)).astype(np.float32)
    y = m.pcm_pitch(device, [x], 4, 1.0)[0].astype(np.float64)
    r = m.pitch_ratio(4)
    s1 = float(np.float32(1.0) / np.float32(r))
    assert y.size == math.ceil(math.ceil(x.size / s1) / r) and abs(y.size - x.size) <= 2
    peak_hz = np.abs(np.fft.rfft(y * np.hanning(y.size))).argmax() * 44100.0 / y.size
    print(f"+4 semitones: peak {peak_hz:.2f} Hz, wanted {220.0 * 2 ** (4 / 12):.2f} (bin {44100.0 / y.size:.2f} Hz)")
    assert abs(peak_hz - 220.0 * 2 ** (4 / 12)) <= 44100.0 / y.size


@pytest.mark.parametrize("st, speed, named", [(12.5, 1.0, "12.5"), (float("nan"), 1.0, "nan"), (-12.0, 2.0, "time-scale of 4")])
def test_refused(device, st, speed, named):
    with pytest.raises(m.HipError, match=f"rc=-6: .*{named}"):
        m.pcm_pitch(device, [X[:100]], st, speed)


def miotts(tool, files, *extra):
    return subprocess.run([os.path.join(BIN, tool), "-c", files["codec"], "-v", files["voice"], "--skip-llm", "-p",
                           files["prompt"]] + [str(a) for a in extra], capture_output=True, text=True, timeout=120)


def test_miotts_pitch(device, tmp_path):
    codes = np.random.default_rng(5).integers(0, 12800, 30).astype(np.int32)
    files = {"codec": m.synth_codec(str(tmp_path / "codec_tiny.gguf"), 1, 1),
             "voice": m.synth_voice(str(tmp_path / "voice.emb.gguf"), 7), "prompt": "".join(f"<|s_{c}|>" for c in codes)}
    for name, extra in {"up": ["--pitch", 3], "zero": ["--pitch", 0], "plain": []}.items():
        p = miotts("miotts", files, "-o", tmp_path / f"{name}.wav", *extra)
        assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "zero.wav").read_bytes() == (tmp_path / "plain.wav").read_bytes()
    pcm = m.Codec(device, files["codec"]).decode_pcm(codes, m.read_voice(files["voice"]))
    y = m.pcm_pitch(device, [pcm], 3)[0]
    want, _ = m.pcm_finish(device, device.upload(y), y.size, True)
    with wave.open(str(tmp_path / "up.wav")) as w:
        got = np.frombuffer(w.readframes(w.getnframes()), np.int16)
    np.testing.assert_array_equal(got, want)
    for tool, pitch in [("miotts", 12.5), ("miotts-stream-benchmark", 3), ("miotts-stream-compare", 3)]:
        p = miotts(tool, files, "--pitch", pitch)
        assert p.returncode == 1 and "--pitch" in p.stderr, (tool, pitch, p.stderr[-500:])
