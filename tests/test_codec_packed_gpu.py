"""GPU parity: the packed MioCodec decode (mio_hip_codec_decode_pcm_packed: B utterances of
different lengths and voices concatenated along the row axis, csrc/hip/codec_packed.hip) against
the float64 numpy restatement (tests/np_codec.py) run per utterance with its own embedding.

Bounds are those of the single decode (test_codec_gpu.py, whose docstring derives them), applied
to every utterance on its own:
  * F32 preset: per stage RMS(diff) <= 1e-3 RMS(ref) and max|diff| <= 5e-3 max|ref|;
                PCM RMS(diff) <= 1e-4 absolute and <= 1e-3 RMS(ref);
  * F16 preset: stages before the spectrogram 3e-3 / 1e-2, spectrogram and PCM 5e-3 of their RMS.
Every test prints its worst err / bound before it asserts.
"""
import functools
import os
import subprocess
import wave

import numpy as np
import pytest

import miotts_amd as m
import np_codec
import pyoracle

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "miotts-llama.cpp_amd", "build")
HALF = 65 // 2   # half the band window of the tiny presets (prenet and decoder)
TAPS = 3         # the widest tap window: the ResNet convs and the k = 7, stride 3 ConvT
# Length sets, each the smallest at which one boundary rule can fail. The M-tile of the segment
# GEMM and of the segment conv is 64 rows (SG_T, CV_BM = kSegConvTileM), an attention workgroup
# holds 16 queries: [5, 20, 9] puts the decoder-resolution boundaries (rows 10 and 50) strictly
# inside the first tile; [32, 7] puts one exactly on a tile edge at every resolution (rows 64,
# 192, 576) and on an attention-block edge (code 32).
LENS = [[1], [1, 1, 1], [HALF + 2, 2, HALF + 2], [TAPS - 1, 40], [5, 20, 9], [32, 7], list(range(1, 17))]


@functools.lru_cache(maxsize=None)
def _files(tmp, preset):
    return m.synth_codec(os.path.join(tmp, f"codec{preset}.gguf"), preset, 1)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("codec_packed"))


def _inputs(lens, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    codes = [rng.integers(0, 12800, n).astype(np.int32) for n in lens]
    embs = [(scale * rng.standard_normal(128)).astype(np.float32) for _ in lens]
    return codes, embs


@functools.lru_cache(maxsize=None)
def _reference(path, lens, seed):
    """np_codec per utterance: [utterance][stage] float64, and the PCM of its spectrogram."""
    nc = np_codec.Codec(path)
    codes, embs = _inputs(lens, seed)
    st = [nc.stages(c, e) for c, e in zip(codes, embs)]
    pcm = [pyoracle.istft(s[-1].astype(np.float32).reshape(len(s[-1]), -1, 2)) for s in st]
    return st, pcm


def _rel(g, o):
    """(RMS(diff) / RMS(ref), max|diff| / max|ref|, RMS(diff), RMS(ref))"""
    assert g.shape == o.shape, (g.shape, o.shape)
    d = g.astype(np.float64) - o.astype(np.float64)
    rms, rms_ref = np.sqrt(np.mean(d * d)), np.sqrt(np.mean(o.astype(np.float64) ** 2))
    return rms / (rms_ref + 1e-30), np.abs(d).max() / (np.abs(o).max() + 1e-30), rms, rms_ref


def _stage_ratio(g, o, f16, last):
    """worst err / bound of one utterance's stage"""
    rr, rm, _, _ = _rel(g, o)
    if f16 and last:
        return rr / 5e-3
    return max(rr / (3e-3 if f16 else 1e-3), rm / (1e-2 if f16 else 5e-3))


def _pcm_ratio(g, o, f16):
    rr, _, rms, _ = _rel(g, o)
    return rr / 5e-3 if f16 else max(rms / 1e-4, rr / 1e-3)


@pytest.mark.parametrize("preset", [1, 2], ids=["f32", "f16"])
@pytest.mark.parametrize("lens", LENS, ids=lambda l: "-".join(map(str, l)) if len(l) < 9 else "1to16")
def test_packed_parity(device, tmp, preset, lens):
    """Every stage and the PCM of every utterance of a packed decode against np_codec."""
    path = _files(tmp, preset)
    gc = m.Codec(device, path)
    codes, embs = _inputs(lens, 3)
    ref, ref_pcm = _reference(path, tuple(lens), 3)
    n_stages, cap = len(ref[0]), 18 * sum(lens) * 512 + 4096
    worst = 0.0
    for st in range(n_stages):
        got = gc.decode_stage_packed(codes, embs, st, cap)
        for b in range(len(lens)):
            worst = max(worst, _stage_ratio(got[b], ref[b][st], preset == 2, st == n_stages - 1))
    pcm = gc.decode_pcm_packed(codes, embs)
    worst_pcm = max(_pcm_ratio(pcm[b], ref_pcm[b], preset == 2) for b in range(len(lens)))
    print(f"packed preset {preset} lens {lens}: worst stage err/bound {worst:.3g}, PCM {worst_pcm:.3g}")
    assert all(len(p) == n * gc.samples_per_token for p, n in zip(pcm, lens))
    assert worst <= 1.0 and worst_pcm <= 1.0, (worst, worst_pcm)


@pytest.mark.parametrize("preset", [1, 2], ids=["f32", "f16"])
def test_packed_no_leakage(device, tmp, preset):
    """Utterance 1 of 3 decoded twice with the same codes and voice: once beside neighbours
    with N(0, 1) voices, once beside neighbours whose voices are scaled by 50 and whose codes
    are others. The lengths are the same, so every kernel cuts its tiles, slices and windows the
    same way, and a row reads its own segment only: its rows at every stage and its PCM are
    equal bit for bit. The reference's neighbour outputs move by more than 100 bounds between
    the two runs, so the equality is not vacuous."""
    path = _files(tmp, preset)
    gc = m.Codec(device, path)
    lens = (9, 21, 6)
    ca, ea = _inputs(lens, 11)
    cb, eb = _inputs(lens, 12, 50.0)
    cb[1], eb[1] = ca[1], ea[1]
    nc = np_codec.Codec(path)
    moved = _rel(nc.stages(cb[0], eb[0])[-1], _reference(path, lens, 11)[0][0][-1])[0]
    print(f"reference neighbour spectrogram moved by {moved:.3g} of its RMS")
    assert moved >= 100 * 5e-3
    cap = 18 * sum(lens) * 512 + 4096
    for st in range(len(_reference(path, lens, 11)[0][0])):
        a, b = gc.decode_stage_packed(ca, ea, st, cap), gc.decode_stage_packed(cb, eb, st, cap)
        assert np.array_equal(a[1], b[1]), st
    assert np.array_equal(gc.decode_pcm_packed(ca, ea)[1], gc.decode_pcm_packed(cb, eb)[1])


@pytest.mark.parametrize("preset", [1, 2], ids=["f32", "f16"])
@pytest.mark.parametrize("lens", [(13, 40, 7), (13, 700, 7)], ids=["short", "mixed_kgroups"])
def test_packed_against_single_decode(device, tmp, preset, lens):
    """Three utterances with three voices: each PCM against mio_hip_codec_decode_pcm of the
    same codes and voice, to the PCM bound of the single decode. Every packed GEMM runs with the
    K-groups its segment's single decode takes and every other kernel sums in the single
    decode's order, so the PCM is also equal bit for bit; (13, 700, 7) puts the utterances into
    different K-group runs (4 / 2 / 1 K-groups at the upsampler, out_proj and head GEMMs).
    Measured worst err / bound: 0 (both presets, both length sets)."""
    gc = m.Codec(device, _files(tmp, preset))
    codes, embs = _inputs(lens, 21)
    got = gc.decode_pcm_packed(codes, embs)
    want = [gc.decode_pcm(c, e) for c, e in zip(codes, embs)]
    worst = max(_pcm_ratio(g, w, preset == 2) for g, w in zip(got, want))
    print(f"packed against single decode, preset {preset} lens {lens}: worst PCM err/bound {worst:.3g}")
    assert worst <= 1.0, worst
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("case", ["B=0", "B=17", "null_emb", "bad_code"])
def test_packed_refusals(device, tmp, case):
    """A refused packed call (checked before anything is allocated or queued) and then a valid
    one on the same handle, which gives what it gave before the refusal."""
    gc = m.Codec(device, _files(tmp, 1))
    codes, embs = _inputs((4, 9, 3), 31)
    before = gc.decode_pcm_packed(codes, embs)
    bad_c, bad_e = [c.copy() for c in codes], list(embs)
    if case == "B=0":
        bad_c, bad_e = [], []
    elif case == "B=17":
        bad_c, bad_e = [codes[0]] * 17, [embs[0]] * 17
    elif case == "null_emb":
        bad_e[1] = None
    else:
        bad_c[2][1] = gc.n_codes
    with pytest.raises(m.HipError, match={"B=0": "utterances outside", "B=17": "utterances outside",
                                          "null_emb": "utterance 1", "bad_code": "utterance 2"}[case]):
        gc.decode_pcm_packed(bad_c, bad_e)
    after = gc.decode_pcm_packed(codes, embs)
    for a, b, c, e in zip(after, before, codes, embs):
        assert np.array_equal(a, b) and _pcm_ratio(a, gc.decode_pcm(c, e), False) <= 1.0


def test_stage_probe_refuses_small_buffer(device, tmp):
    """The stage probe writes nothing into a buffer smaller than the stage; a probe with room
    for it gives the same rows afterwards."""
    gc = m.Codec(device, _files(tmp, 1))
    codes, embs = _inputs((4, 9, 3), 31)
    before = gc.decode_stage_packed(codes, embs, 0, 16 * 4096)  # stage 0: 16 rows of the prenet width
    with pytest.raises(m.HipError, match="room for"):
        gc.decode_stage_packed(codes, embs, 0, before[0].shape[1] * 16 - 1)
    after = gc.decode_stage_packed(codes, embs, 0, before[0].shape[1] * 16)
    assert all(np.array_equal(a, b) for a, b in zip(after, before))


def _wav(path):
    with wave.open(str(path)) as w:
        return np.frombuffer(w.readframes(w.getnframes()), np.int16).astype(np.int32)


def test_miotts_batch_voices(tmp_path):
    """`miotts --batch FILE --voices FILE2`: line i is spoken by the voice on line i of FILE2,
    the codec decodes packed; a packed utterance is bit-equal to its single decode
    (test_packed_against_single_decode), so every WAV has the bytes of the single run with that
    voice. A --voices file with another line count is refused with exit status 1."""
    d = tmp_path
    llm, codec = m.synth_llm(str(d / "llm.gguf"), 1, 1), m.synth_codec(str(d / "codec.gguf"), 1, 1)
    voices = [m.synth_voice(str(d / f"v{i}.emb.gguf"), 7 + i) for i in range(2)]
    prompts = ["テストです。", "こんにちは。"]
    (d / "batch.txt").write_text("\n".join(prompts) + "\n", "utf-8")
    (d / "voices.txt").write_text("\n".join(voices) + "\n", "utf-8")
    common = [os.path.join(BIN, "miotts"), "-m", llm, "-c", codec, "--max-tokens", "24", "--speech-only",
              "--ignore-eos"]
    p = subprocess.run(common + ["-v", voices[0], "--batch", str(d / "batch.txt"), "--voices", str(d / "voices.txt"),
                                 "-o", str(d / "b.wav")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "batched decode unavailable" not in p.stderr, p.stderr[-2000:]
    lsb = []
    for i, (text, v) in enumerate(zip(prompts, voices)):
        s = subprocess.run(common + ["-v", v, "-p", text, "-o", str(d / f"s{i}.wav")], capture_output=True,
                           text=True, timeout=300)
        assert s.returncode == 0, s.stderr[-2000:]
        a, b = _wav(d / f"b_{i:03d}.wav"), _wav(d / f"s{i}.wav")
        assert a.shape == b.shape, i
        lsb.append(int(np.abs(a - b).max()))
    print(f"miotts --voices against single runs: max |diff| {lsb} LSB of PCM16")
    assert max(lsb) <= 1, lsb
    for i in range(len(prompts)):
        assert (d / f"b_{i:03d}.wav").read_bytes() == (d / f"s{i}.wav").read_bytes(), i
    assert not np.array_equal(_wav(d / "b_000.wav")[:1000], _wav(d / "b_001.wav")[:1000])
    (d / "one.txt").write_text(voices[0] + "\n", "utf-8")
    p = subprocess.run(common + ["-v", voices[0], "--batch", str(d / "batch.txt"), "--voices", str(d / "one.txt"),
                                 "-o", str(d / "x.wav")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "--voices" in p.stderr, (p.returncode, p.stderr[-500:])
