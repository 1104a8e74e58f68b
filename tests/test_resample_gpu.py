"""GPU: the output-rate resampler (csrc/hip/pcm_resample.hip) against the float64 sum over the
handle's own table, its bit-equalities, its filter on tones, and the rate through miotts and the stream.
The indexing, restated once: y[n] = sum_t x[n M // L - P/2 + 1 + t] * c[n M % L][P - 1 - t], x = 0
outside the signal, ceil(N L / M) outputs. The bound per output is the first-order bound of a
P-term f32 FMA chain, gamma = (P + 1) 2^-24 sum_t |x_t c_t|."""
import math
import os
import subprocess
import wave

import numpy as np
import pytest

import miotts_amd as m

pytestmark = pytest.mark.gpu

BIN = os.path.join(m.PKG_ROOT, "build")
RATES = [48000, 16000, 22050, 8000]  # an up ratio, the largest table, L = 1, the longest P
SIZES = ["one", "half_p", "p", "tile_minus", "tile_plus", "long"]


def reference(x, c, L, M):
    P = c.shape[1]
    n = np.arange(-(-len(x) * L // M))
    xp = np.concatenate([np.zeros(P), x.astype(np.float64), np.zeros(P)])  # x[i] at xp[i + P]
    terms = xp[(n * M // L)[:, None] - P // 2 + 1 + np.arange(P)[None, :] + P] * c[n * M % L][:, ::-1]
    return terms.sum(1), np.abs(terms).sum(1)


def to_pcm16(s):
    t = s.astype(np.float32) * np.float32(32767.0)
    return np.trunc(np.clip(t, np.float32(-32768.0), np.float32(32767.0))).astype(np.int32).astype(np.int16)


def in_pieces(rs, x, cuts, **kw):
    out, i = [], 0
    for k in cuts:
        k = min(k, len(x) - i)
        if k:
            out.append(rs(x[i:i + k], **kw))
        i += k
    out.append(rs(x[i:], flush=True, **kw))
    return np.concatenate(out)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("f_out", RATES)
def test_parity_chunking_and_fusion(device, f_out, size):
    rs = m.Resampler(device, 44100, f_out)
    L, M, P = rs.L, rs.M, rs.P
    n = {"one": 1, "half_p": P // 2, "p": P, "tile_minus": rs.tile * M // L - 1, "tile_plus": rs.tile * M // L + 1,
         "long": 20000}[size]
    rng = np.random.default_rng(f_out + n)
    x = (rng.standard_normal(n) * 0.3).astype(np.float32)
    k = min(n, 16)
    x[:k] += np.linspace(1.0, 0.0, k, dtype=np.float32)   # +-1.0 at the two ends: the zero extension
    x[n - k:] -= np.linspace(0.0, 1.0, k, dtype=np.float32)
    # against float64
    y = rs(x, flush=True)
    want, mag = reference(x, rs.coeffs().astype(np.float64), L, M)
    assert y.shape == want.shape == (math.ceil(n * L / M),)
    err, gamma = np.abs(y - want), (P + 1) * 2.0 ** -24 * mag
    print(f"{f_out} Hz n={n}: worst err / gamma = {(err / np.maximum(gamma, 1e-300)).max():.3f}")
    assert (err <= gamma).all()
    # chunking: the cut of the stream into calls changes no bit
    cuts = (1, 7, P - 1, 4097)
    np.testing.assert_array_equal(in_pieces(rs, x, cuts).view(np.uint32), y.view(np.uint32))
    y16 = rs(x, flush=True, pcm16=True)
    np.testing.assert_array_equal(y16, to_pcm16(y))
    np.testing.assert_array_equal(in_pieces(rs, x, cuts, pcm16=True), y16)
    # fusion: peak pass + one launch equals normalise, resample to floats, convert
    d = device.upload(x)
    fused, peak = rs.finish(d, n, True)
    m.check(m.lib().mio_hip_pcm_normalize(device.h, d.ptr, n, d.ptr, None, None))
    assert peak == np.abs(x).max()
    np.testing.assert_array_equal(fused, to_pcm16(rs(d.numpy(), flush=True)))


@pytest.mark.parametrize("f_out", RATES)
def test_one_khz_tone_comes_out_at_one_khz(device, f_out):
    """The steady part fits a 1 kHz sinusoid at the output rate with the passband's gain (+-0.002 dB),
    leaving at most the L - 1 images of the tone, each <= -79 dB: sqrt(L) 10^(-79/20) of its RMS."""
    rs = m.Resampler(device, 44100, f_out)
    y = rs(np.sin(2 * np.pi * 1000.0 / 44100 * np.arange(20000)).astype(np.float32), flush=True).astype(np.float64)
    edge = max(rs.P // 2, math.ceil(rs.P / 2 * rs.L / rs.M))
    t = np.arange(y.size)[edge:-edge] / f_out
    A = np.stack([np.sin(2 * np.pi * 1000.0 * t), np.cos(2 * np.pi * 1000.0 * t)], 1)
    coef, *_ = np.linalg.lstsq(A, y[edge:-edge], rcond=None)
    resid = np.sqrt(np.mean((y[edge:-edge] - A @ coef) ** 2)) * np.sqrt(2.0)
    gain_db = 20 * np.log10(np.hypot(*coef))
    print(f"{f_out} Hz: gain {gain_db:+.5f} dB, residual {resid:.3g} of the tone's RMS")
    assert abs(gain_db) <= 0.002 and resid <= np.sqrt(rs.L) * 10 ** (-79 / 20)


def test_fifteen_khz_tone_is_gone_at_16_khz(device):
    rs = m.Resampler(device, 44100, 16000)
    x = np.sin(2 * np.pi * 15000.0 / 44100 * np.arange(20000)).astype(np.float32)
    y = rs(x, flush=True).astype(np.float64)
    edge = max(rs.P // 2, math.ceil(rs.P / 2 * rs.L / rs.M))
    db = 20 * np.log10(np.sqrt(np.mean(y[edge:-edge] ** 2)) / np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    print(f"15 kHz into 16 kHz: {db:.2f} dB")
    assert db <= -79.0


def run(args):
    p = subprocess.run([os.path.join(BIN, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, f"{args[0]} rc={p.returncode}\n{p.stdout}\n{p.stderr[-2000:]}"
    assert "batched decode unavailable" not in p.stderr, p.stderr[-2000:]
    return p.stdout


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("rate")
    return {"llm": m.synth_llm(str(d / "llm1.gguf"), 1, 1), "codec": m.synth_codec(str(d / "codec_tiny.gguf"), 1, 1),
            "voice": m.synth_voice(str(d / "voice.emb.gguf"), 7), "dir": d}


def test_miotts_sample_rate_16000(device, files):
    codes = np.random.default_rng(3).integers(0, 12800, 40).astype(np.int32)
    wav = files["dir"] / "r16.wav"
    run(["miotts", "-c", files["codec"], "-v", files["voice"], "--skip-llm", "-p", "".join(f"<|s_{c}|>" for c in codes),
         "-o", wav, "--sample-rate", 16000])
    pcm = m.Codec(device, files["codec"]).decode_pcm(codes, m.read_voice(files["voice"]))
    with wave.open(str(wav)) as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        got = np.frombuffer(w.readframes(w.getnframes()), np.int16)
    assert got.size * 2 == math.ceil(pcm.size * 160 / 441) * 2
    want, _ = m.Resampler(device, 44100, 16000).finish(device.upload(pcm), pcm.size, True)
    np.testing.assert_array_equal(got, want)
    p = subprocess.run([os.path.join(BIN, "miotts"), "-c", files["codec"], "-v", files["voice"], "--skip-llm", "-p",
                        "<|s_1|>", "--sample-rate", "12000"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "12000" in p.stderr


def test_miotts_batch_at_16000_equals_single_runs(files):
    d = files["dir"]
    prompts = ["テストです。", "こんにちは。", "今日はいい天気ですね。"]
    (d / "batch.txt").write_text("\n".join(prompts) + "\n", "utf-8")
    common = ["-m", files["llm"], "-c", files["codec"], "-v", files["voice"], "--max-tokens", 24, "--speech-only",
              "--ignore-eos", "--sample-rate", 16000]
    run(["miotts"] + common + ["--batch", d / "batch.txt", "-o", d / "b.wav"])
    for i, p in enumerate(prompts):
        run(["miotts"] + common + ["-p", p, "-o", d / f"s{i}.wav"])
        assert (d / f"b_{i:03d}.wav").read_bytes() == (d / f"s{i}.wav").read_bytes(), i


def test_stream_at_48000_is_the_native_stream_resampled(device, files):
    """A 48 kHz stream's chunks, concatenated, against the stateful handle fed the chunks the same
    run emits at the codec's rate (the sampler is counter-based: the run repeats)."""
    common = ["miotts-stream-benchmark", "-m", files["llm"], "-c", files["codec"], "-v", files["voice"], "-p",
              "こんにちは、今日はいい天気ですね。", "--max-tokens", 100, "--speech-only", "--ignore-eos",
              "--chunk-samples", 1000, "--dump-stream"]
    native, rated = str(files["dir"] / "native"), str(files["dir"] / "r48")
    run(common + [native])
    out = run(common + [rated, "--sample-rate", 48000])
    x, cuts = np.fromfile(native + ".f32", np.float32), np.fromfile(native + ".chunks.i64", np.int64)
    got = np.fromfile(rated + ".f32", np.float32)
    assert cuts.sum() == x.size and got.size == math.ceil(x.size * 160 / 147)
    assert f"stream_bench.emitted_samples={got.size}\n" in out
    want = in_pieces(m.Resampler(device, 44100, 48000), x, [int(c) for c in cuts])
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
