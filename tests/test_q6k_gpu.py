"""GPU parity: all-Q6_K GGUF files (MOSTLY_Q6_K: ggml type 14 in every role) on every LLM path.

Type 14 ran before as attn_v / ffn_down / output beside Q4_K or Q5_K only. Here it is q|k, O and
gate|up too: the row pairs and SwiGLU epilogue of the gate|up launches, the fused single-stream
launches (k_layer_att, k_ffn) and the batched decode's in-launch quantization.

 * row pairs: silu(g) * u of the decode stream and of the int8-MFMA matmul against the two plain
   products in float64 (expf differs from numpy's exp by an ulp: 1e-5 * max + 1e-6, the bound
   test_q5k_gpu.py puts on the same epilogue); the matmul's modes 0 / 1 equal the single-token
   matvec BIT FOR BIT;
 * layer by layer against the C oracle on the GPU's own layer input and K/V rows (conv ring for
   lfm2): test_llm_layers_gpu.py's scheme and its bounds for the integer types;
 * batched prefill, batched decode and the fused launches equal the single-token decode and
   the separate launches BIT FOR BIT;
 * the launch structure of the 1.7B / 2.6B / 0.1B shapes as Q6_K is the one their Q4_K_M / Q8_0
   presets have (step_kinds, batch_step_launches).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import miotts_amd as m
import pyoracle

pytestmark = pytest.mark.gpu

ALLOW = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "miotts-llama.cpp_amd", "build")


@pytest.fixture(scope="session")
def q6k_path(tmp_path_factory):
    """q6k_path(preset) -> the preset's shape written as MOSTLY_Q6_K (seed 1), once per session."""
    d = tmp_path_factory.mktemp("q6k_models")
    cache = {}

    def get(preset: int) -> str:
        if preset not in cache:
            cache[preset] = m.synth_llm_as(str(d / f"llm{preset}_q6k.gguf"), preset, 18, 1)
        return cache[preset]

    return get


def _silu_mul(g, u):
    g = g.astype(np.float64)
    return g / (1.0 + np.exp(-g)) * u.astype(np.float64)


# ------------------------------------------------------------------ row pairs
# k: a partial pass (256, 768), one full pass (2048), a pass boundary (2304) and three passes (6144)
@pytest.mark.parametrize("k", [256, 768, 2048, 2304, 6144])
def test_matvec_swiglu_row_pairs(device, k):
    rng = np.random.default_rng(14000 + k)
    rows = 37
    wg = m.quantize_rows(14, (rng.standard_normal((rows, k)) * 0.05).astype(np.float32))
    wu = m.quantize_rows(14, (rng.standard_normal((rows, k)) * 0.05).astype(np.float32))
    x = rng.standard_normal(k).astype(np.float32)
    x[3] = -9.0
    y = m.debug_matvec_swiglu(device, 14, wg, wu, k, x)
    want = _silu_mul(m.debug_matvec(device, 14, wg, k, x), m.debug_matvec(device, 14, wu, k, x))
    err = float(np.abs(y - want).max())
    print(f"k {k}: max err {err:.3g}, max|want| {np.abs(want).max():.3g}")
    assert err <= 1e-5 * float(np.abs(want).max()) + 1e-6


# the last shape has more 16-row tiles than the chip has CUs: the tile-walking kernel
@pytest.mark.parametrize("k,rows,nt", [(256, 50, 3), (2048, 70, 8), (2048, 70, 32), (6144, 33, 16), (6144, 32, 40),
                                       (2048, 4200, 6)])
def test_mmq_equals_single_token_matvec(device, k, rows, nt):
    rng = np.random.default_rng(14 * 7 + k + nt)
    wq = m.quantize_rows(14, (rng.standard_normal((rows, k)) * 0.05).astype(np.float32))
    x = rng.standard_normal((nt, k)).astype(np.float32)
    x[:, 3] = -9.0
    y0 = m.debug_mmq(device, 14, wq, k, x)
    refs = [m.debug_matvec(device, 14, wq, k, x[t]) for t in range(nt)]
    for t in range(nt):
        assert np.array_equal(y0[t], refs[t]), (t, float(np.abs(y0[t] - refs[t]).max()))
    r0 = rng.standard_normal((nt, rows)).astype(np.float32)
    y = m.debug_mmq(device, 14, wq, k, x, mode=1, y_in=r0)
    for t in range(nt):
        assert np.array_equal(y[t], refs[t] + r0[t]), t
    wu = m.quantize_rows(14, (rng.standard_normal((rows, k)) * 0.05).astype(np.float32))
    u0 = m.debug_mmq(device, 14, wu, k, x)
    y = m.debug_mmq(device, 14, wq, k, x, mode=2, up_rows=wu)
    for t in range(nt):
        want = _silu_mul(y0[t], u0[t])
        err = float(np.abs(y[t] - want).max())
        assert err <= 1e-5 * float(np.abs(want).max()) + 1e-6, (t, err)


# ------------------------------------------------------------------ layers against the oracle
POSITIONS = (0, 5, 63, 64, 65, 129)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


# 1 qwen3, 8 lfm2, 9 the 576 width (Q8_0 + a Q6_K down), 17 the 1.7B head shape (hd 128, G 2)
@pytest.mark.parametrize("preset", [1, 8, 9, 17])
def test_layers_match_oracle_on_gpu_inputs(device, q6k_path, preset):
    """test_llm_layers_gpu.py's scheme at n_ctx 256: each layer of the oracle gets the GPU's layer
    input and the GPU's K/V rows of the positions before (lfm2 short conv: the GPU's ring)."""
    path = q6k_path(preset)
    g = m.Llm(device, path, 256)
    o = pyoracle.Llm(path, POSITIONS[-1] + 8)
    rng = np.random.default_rng(1400 + preset)
    toks = [256, 257] + [int(t) for t in rng.integers(m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800, POSITIONS[-1])]
    errs, kv_bad = [], []
    for pos in range(POSITIONS[-1] + 1):
        if pos not in POSITIONS:
            g.eval(toks[pos], pos)
            continue
        xs, _ = g.eval_layers(toks[pos], pos)
        assert np.array_equal(xs[0], o.embed(toks[pos]))  # a Q6_K (preset 9: Q8_0) embedding row
        for il in range(g.n_layer):
            if o.is_conv(il):
                ring = g.conv_ring(il)
                o.set_conv_ring(il, ring)
                y = o.layer(il, pos, xs[il])
                errs.append((_rel(xs[il + 1], y), pos, il))
                kv_bad.append(int(_rel(ring[pos & 3], o.conv_ring(il)[pos & 3]) > 1e-5))
                continue
            if pos:
                k, v = g.kv_rows(il, pos)
                o.set_kv(il, k, v)
            y = o.layer(il, pos, xs[il])
            errs.append((_rel(xs[il + 1], y), pos, il))
            kg, vg = g.kv_rows(il, pos + 1)
            ko, vo = o.kv(il, pos + 1)
            off = 0
            for a, b in ((kg[:, pos], ko[:, pos]), (vg[:, pos], vo[:, pos])):
                ulp = np.abs(np.spacing(b)).astype(np.float64)
                off += int((np.abs(a.astype(np.float64) - b.astype(np.float64)) > ulp + 1e-12).sum())
            kv_bad.append(off)
    g.close()
    e = np.array([x[0] for x in errs])
    worst = max(errs)
    by_layer, by_pos = {}, {}
    for v, pos, il in errs:
        by_layer.setdefault(il, []).append(v)
        by_pos.setdefault(pos, []).append(v)
    worst_layer = max((np.median(v), il) for il, v in by_layer.items())
    worst_pos = max((np.median(v), pos) for pos, v in by_pos.items())
    n_kv_bad = sum(1 for b in kv_bad if b)
    print(f"preset {preset} as Q6_K: {len(e)} layer evaluations, median {np.median(e):.3g}, max {worst[0]:.3g} "
          f"(pos {worst[1]}, layer {worst[2]}), > 1e-4: {(e > 1e-4).sum()}, worst per-layer median "
          f"{worst_layer[0]:.3g} (layer {worst_layer[1]}), worst per-position median {worst_pos[0]:.3g} "
          f"(pos {worst_pos[1]}), K/V rows off by > 1 ulp: {n_kv_bad} of {len(kv_bad)}")
    assert worst_layer[0] <= 1e-5 and worst_pos[0] <= 1e-5, (worst_layer, worst_pos)
    assert (e > 1e-4).sum() <= 0.12 * len(e)
    assert worst[0] <= 5e-2, worst
    assert n_kv_bad <= 0.12 * len(kv_bad), kv_bad


# ------------------------------------------------------------------ prefill / batch == decode
@pytest.mark.parametrize("preset,n", [(1, 2), (1, 40), (1, 150), (9, 17)])
def test_batched_prefill_matches_sequential(device, q6k_path, preset, n):
    g = m.Llm(device, q6k_path(preset), 256)
    toks = np.random.default_rng(140 + n).integers(0, g.n_vocab, n)
    batched = g.prefill(toks)
    seq = None
    for pos, t in enumerate(toks):
        seq = g.eval(int(t), pos)
    g.close()
    assert np.array_equal(batched, seq), float(np.abs(batched - seq).max())


def _prompts(B, seed):
    rng = np.random.default_rng(seed)
    lens = [1 if b == 1 else int(rng.integers(3, 40)) for b in range(B)]  # a 1-token prompt too
    return [list(rng.integers(0, 256, n)) for n in lens]


# B = 3: the launches that quantize their input themselves; B = 9: plain 16-token tiles
@pytest.mark.parametrize("B", [3, 9])
def test_batch_equals_single_streams(device, q6k_path, B):
    g = m.Llm(device, q6k_path(1), 256)
    prompts = _prompts(B, 140 + B)
    seeds = [1400 + 17 * b for b in range(B)]
    got = g.generate_batch(prompts, 24, 0.8, seeds, allow=ALLOW)
    for b in range(B):
        ref = g.generate(prompts[b], 24, 0.8, seeds[b], allow=ALLOW)
        assert np.array_equal(got[b], ref), (b, got[b], ref)
    g.close()


# ------------------------------------------------------------------ the full-size shapes
_FUSION_SCRIPT = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, sys.argv[2])
import miotts_amd as m
dev = m.Device(0)
g = m.Llm(dev, sys.argv[1], 256)
prompt = np.array([256, 257, 65, 258, 257, 300, 301], np.int32)
toks = g.generate(prompt, 40, 0.8, 5, allow=(m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800), check_interval=16)
h = hashlib.sha256(toks.tobytes())
h.update(g.eval(int(toks[0]), 70).tobytes())
k = g.step_kinds()
print(k.count(11), k.count(12), len(toks), h.hexdigest())
"""

_SEPARATE = {"MIO_LAYER_ATT": "0", "MIO_ATT_FUSE_O": "0", "MIO_FFN_FUSE": "0"}


def _fused_vs_separate(path, tmp_path):
    """Two fresh processes (the switches are read once), one with the three fusion switches at 0:
    each prints its kind-11 / kind-12 counts, the token count and a SHA-256 over 40 generated
    tokens plus one eval row."""
    script = tmp_path / "fusion.py"
    script.write_text(_FUSION_SCRIPT)
    pkg = os.path.dirname(os.path.dirname(m.__file__))
    outs = {}
    for name, env in (("fused", {}), ("separate", _SEPARATE)):
        p = subprocess.run([sys.executable, str(script), path, pkg], capture_output=True, text=True, timeout=240,
                           env=dict(os.environ, **env))
        assert p.returncode == 0, p.stderr[-2000:]
        outs[name] = p.stdout.split()
    print(outs)
    assert int(outs["separate"][0]) == 0 and int(outs["separate"][1]) == 0
    assert int(outs["fused"][2]) == 40 and int(outs["separate"][2]) == 40
    assert outs["fused"][3] == outs["separate"][3], outs
    return int(outs["fused"][0]), int(outs["fused"][1])


def _kinds(device, path):
    g = m.Llm(device, path, 256)
    k = g.step_kinds()
    g.close()
    return k.count(11), k.count(12)


def test_fused_launches_1p7b_q6k(device, synth_llm_path, q6k_path, tmp_path):
    """The 1.7B shape as Q6_K runs the attention block and the FFN pair as one launch each on as
    many layers as preset 3 (Q4_K_M) does, and its batched step issues as many launches; a
    68-token prefill and a 4-stream batched decode (the q|k|v and gate|up launches quantizing
    in the launch, the gate|up tile walk, the three-pass down) equal the single-token decode;
    the fused launches are bit-identical with the separate ones."""
    g3 = m.Llm(device, synth_llm_path(3), 256)
    kinds3 = g3.step_kinds()
    launches3 = g3.batch_step_launches(4)
    g3.close()
    path = q6k_path(3)
    g = m.Llm(device, path, 256)
    kinds = g.step_kinds()
    launches = g.batch_step_launches(4)
    print(f"kinds 11 / 12: {kinds.count(11)} / {kinds.count(12)} (Q4_K_M {kinds3.count(11)} / {kinds3.count(12)}), "
          f"{len(kinds)} launches per step (Q4_K_M {len(kinds3)}); batched step of 4: {launches} (Q4_K_M {launches3})")
    assert kinds.count(11) == kinds3.count(11) > 0 and kinds.count(12) == kinds3.count(12) > 0
    assert launches == launches3 > 0
    toks = np.random.default_rng(68).integers(0, 151936, 68)
    batched = g.prefill(toks)
    for pos, t in enumerate(toks):
        seq = g.eval(int(t), pos)
    assert np.array_equal(batched, seq), float(np.abs(batched - seq).max())
    prompts = _prompts(4, 18)
    got = g.generate_batch(prompts, 12, 0.8, [42, 43, 44, 45], allow=ALLOW)
    for b in range(4):
        assert np.array_equal(got[b], g.generate(prompts[b], 12, 0.8, 42 + b, allow=ALLOW)), b
    g.close()
    assert _fused_vs_separate(path, tmp_path) == (kinds.count(11), kinds.count(12))


def test_fused_launches_2p6b_q6k(device, synth_llm_path, q6k_path, tmp_path):
    want = _kinds(device, synth_llm_path(4))
    path = q6k_path(4)
    got = _kinds(device, path)
    assert got == want and want[0] > 0 and want[1] > 0, (got, want)
    assert _fused_vs_separate(path, tmp_path) == got


def test_fused_launches_0p1b_q6k(device, synth_llm_path, q6k_path, tmp_path):
    """Q8_0 with a Q6_K down: the FFN pair fused as for preset 2; the attention block stays on
    attn_in + the attention / O launch, as the host policy keeps it for this head shape."""
    want = _kinds(device, synth_llm_path(2))
    path = q6k_path(2)
    got = _kinds(device, path)
    assert got == want and want[0] == 0 and want[1] > 0, (got, want)
    assert _fused_vs_separate(path, tmp_path) == got


# ------------------------------------------------------------------ CLI
def _run(args, timeout=300):
    p = subprocess.run([os.path.join(BIN, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"{args[0]} rc={p.returncode}\n{p.stdout}\n{p.stderr[-2000:]}"
    assert "batched decode unavailable" not in p.stderr, p.stderr[-2000:]
    return p.stdout


def test_miotts_batch_equals_single_runs(q6k_path, tmp_path):
    """tests/test_cli_gpu.py's `miotts --batch` check on an all-Q6_K model with the tiny codec."""
    d = tmp_path
    codec = m.synth_codec(str(d / "codec_tiny.gguf"), 1, 1)
    voice = m.synth_voice(str(d / "voice.emb.gguf"), 7)
    prompts = ["テストです。", "こんにちは。", "今日はいい天気ですね。"]
    (d / "batch.txt").write_text("\n".join(prompts) + "\n", "utf-8")
    common = ["-m", q6k_path(1), "-c", codec, "-v", voice, "--max-tokens", 40, "--speech-only", "--ignore-eos"]
    _run(["miotts"] + common + ["--batch", d / "batch.txt", "-o", d / "b.wav", "--gpus", 1])
    for i, p in enumerate(prompts):
        _run(["miotts"] + common + ["-p", p, "-o", d / f"s{i}.wav"])
        assert (d / f"b_{i:03d}.wav").read_bytes() == (d / f"s{i}.wav").read_bytes(), i
