"""GPU: the speaking rate (csrc/hip/pcm_speed.hip, mio_hip_pcm_speed) against tests/np_speed.py,
the float64 restatement of include/mio_hip.h "speaking rate".

The search is compared by score, not by lag, and teacher-forced: frame m's float64 scores are
formed on the template that follows the GPU's own a_{m-1}. With u = 2^-24, t the template and s_d
the N inputs of lag d, the kernel's dot product is one N-term f32 FMA chain, |err| <= N u sum|t_i
s_d,i| <= N u ||t|| ||s_d|| (Cauchy-Schwarz); divided by ||s_d|| that is N u ||t||. Forming the
normaliser (the energy, the added 1e-12, the square root) and dividing by it are counted as four
more roundings, each moving the score by at most u |c| <= u ||t||. So a score is off by at most
(N + 4) u ||t||, and the lag the GPU prefers can lose to the float64 best by at most twice that:
2 (N + 4) 2^-24 ||t||. (The energy's own N-term chain, of non-negative terms, could in the worst
case add (N / 2) u |c|; the bound is held as stated, and the test prints the loss it measures:
0 on every case so far, the GPU picks the float64 maximum.)
The overlap-add rounds twice (x1 - x2, then the FMA) and uses w[r] = 1 - w[r + Hs] to half an
ulp: at most (2^-23 + 2^-24 + 2^-25) max|x| < 2^-22 max|x|."""
import math
import os
import subprocess
import wave

import numpy as np
import pytest

import miotts_amd as m
import np_speed as ref

pytestmark = pytest.mark.gpu

BIN = os.path.join(m.PKG_ROOT, "build")
SPEEDS = [0.5, 0.8, 1.25, 2.0]
X = ref.voiced()


def check_against_reference(x, s, y, off):
    n_out, p = ref.sizes(len(x), s)
    assert y.shape == (n_out,) == (math.ceil(len(x) / float(np.float32(s))),) and off.shape == p.shape
    assert off[0] == 0 and (off >= -ref.D).all() and (off < ref.D).all()
    want, _, rows = ref.wsola(x, s, forced=off)
    if len(rows):
        lost, bound = rows[:, 1] - rows[:, 0], 2 * (ref.N + 4) * 2.0 ** -24 * rows[:, 2]
        print(f"s={s} n={len(x)}: worst score loss / bound = {(lost / np.maximum(bound, 1e-300)).max():.3g}")
        assert (lost <= bound).all()
        assert (off[1:][rows[:, 2] == 0] == 0).all()  # a silent template: every score ties at 0
    err = np.abs(y - want).max(initial=0.0)
    print(f"s={s} n={len(x)}: max |y - float64| = {err:.3g} of {2.0 ** -22 * np.abs(x).max():.3g}")
    assert err <= 2.0 ** -22 * np.abs(x).max()
    return rows


@pytest.mark.parametrize("n", [1, ref.HS - 1, ref.N, ref.N + ref.D + 1, 5 * ref.N + 37, 30011])
@pytest.mark.parametrize("s", SPEEDS)
def test_offsets_and_pcm(device, s, n):
    x = X[:n]
    (y,), (off,) = m.pcm_speed(device, [x], s)
    rows = check_against_reference(x, s, y, off)
    if n == 30011:  # not vacuous: the float64 search itself moves most frames, and silence is reached
        own = ref.wsola(x, s)[1]
        assert (own[1:] != 0).mean() > 0.5 and (off[1:] != 0).mean() > 0.5 and (rows[:, 2] == 0).any()


@pytest.mark.parametrize("s", SPEEDS)
def test_batch_of_three_lengths(device, s):
    xs = [X[:7000], X[11000:11000 + ref.N + 3], X[9000:20011]]  # the last one crosses the silence
    ys, offs = m.pcm_speed(device, xs, s)
    for x, y, off in zip(xs, ys, offs):
        check_against_reference(x, s, y, off)


def test_speed_one_is_the_identity(device):
    """fma(w, x1 - x2, x2) with x1 == x2 is x2: no ulp is lost, the equality is of bits."""
    ys, offs = m.pcm_speed(device, [X, X[:ref.HS - 1]], 1.0)
    for x, y, off in zip([X, X[:ref.HS - 1]], ys, offs):
        assert not off.any()
        np.testing.assert_array_equal(y.view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("s", [0.75, 1.5])
def test_pitch_is_kept(device, s):
    x = np.sin(2 * np.pi * 220.0 / 44100 * np.arange(44100)).astype(np.float32)
    y = m.pcm_speed(device, [x], s)[0][0].astype(np.float64)
    peak_hz = np.abs(np.fft.rfft(y * np.hanning(y.size))).argmax() * 44100.0 / y.size
    rms = np.sqrt(np.mean(y * y)) / np.sqrt(np.mean(x.astype(np.float64) ** 2))
    print(f"s={s}: peak {peak_hz:.2f} Hz (bin {44100.0 / y.size:.2f} Hz), rms ratio {rms:.4f}")
    assert abs(peak_hz - 220.0) <= 44100.0 / y.size and abs(rms - 1.0) <= 0.01


@pytest.mark.parametrize("s", [0.4, 2.5, float("nan")])
def test_refused_speeds(device, s):
    with pytest.raises(m.HipError, match="nan" if s != s else str(s)):
        m.pcm_speed(device, [X[:100]], s)


def miotts(tool, files, *extra):
    return subprocess.run([os.path.join(BIN, tool), "-c", files["codec"], "-v", files["voice"], "--skip-llm", "-p",
                           files["prompt"]] + [str(a) for a in extra], capture_output=True, text=True, timeout=120)


def test_miotts_speed(device, tmp_path):
    codes = np.random.default_rng(5).integers(0, 12800, 30).astype(np.int32)
    files = {"codec": m.synth_codec(str(tmp_path / "codec_tiny.gguf"), 1, 1),
             "voice": m.synth_voice(str(tmp_path / "voice.emb.gguf"), 7), "prompt": "".join(f"<|s_{c}|>" for c in codes)}
    for name, extra in {"fast": ["--speed", 1.25], "one": ["--speed", 1], "plain": []}.items():
        p = miotts("miotts", files, "-o", tmp_path / f"{name}.wav", *extra)
        assert p.returncode == 0, p.stderr[-2000:]
    assert (tmp_path / "one.wav").read_bytes() == (tmp_path / "plain.wav").read_bytes()
    pcm = m.Codec(device, files["codec"]).decode_pcm(codes, m.read_voice(files["voice"]))
    (y,), _ = m.pcm_speed(device, [pcm], 1.25)
    assert y.size == math.ceil(pcm.size / 1.25)
    want, _ = m.pcm_finish(device, device.upload(y), y.size, True)
    with wave.open(str(tmp_path / "fast.wav")) as w:
        got = np.frombuffer(w.readframes(w.getnframes()), np.int16)
    np.testing.assert_array_equal(got, want)
    for tool, speed in [("miotts", 0.4), ("miotts", 2.5), ("miotts-stream-benchmark", 1.25),
                        ("miotts-stream-compare", 1.25)]:
        p = miotts(tool, files, "--speed", speed)
        assert p.returncode == 1 and "--speed" in p.stderr, (tool, speed, p.stderr[-500:])
