"""GPU parity: Q3_K weights (ggml type 11; Q3_K_S / Q3_K_M / Q3_K_L files) on every LLM path.

The C oracle does not read type 11, so the reference is tests/np_q3k.py (an independent numpy
restatement of the block format) swapped into np_ref.DecodeStep.

 * matvec: the GPU's per-superblock integer sums are exact and only the float sum over
   superblocks is reordered, so against the float64 dequant(w) @ act_q8_k(x) the project's bound
   of test_llm_gpu.py holds: 2e-5 * max|y| + 1e-6; so it does on the ceiling block (every code
   -4, every scale -32) against activation codes that are all -127, the largest integer sums;
 * row pairs: silu(g) * u against the two plain products (expf differs from numpy's exp by an
   ulp: 1e-5 * max + 1e-6, the bound test_q5k_gpu.py / test_q6k_gpu.py put on this epilogue);
 * the int8-MFMA matmul's modes 0 / 1, the batched prefill and the batched decode equal the
   single-token decode BIT FOR BIT (same integer sums, same float terms, same lane / tree order);
 * layer by layer against the numpy layer on the GPU's own layer input and K/V rows (conv ring
   for lfm2): test_q5k_gpu.py's scheme and bounds;
 * the fused launches (attention block, FFN pair) exist for the 1.7B shape as Q3_K_S / _M / _L
   and are bit-identical with the separate launches;
 * IQ4_NL (llama-quantize's fallback for Q3_K rows that are not whole superblocks), Q2_K and a
   Q3_K output matrix stay refused, by the tensor's name and type.
"""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import miotts_amd as m
import np_q3k
import np_ref
from miotts_amd import gguf_np

pytestmark = pytest.mark.gpu

ALLOW = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "miotts-llama.cpp_amd", "build")


@pytest.fixture(scope="session")
def q3k_path(tmp_path_factory):
    """q3k_path(preset, recipe) -> the preset's shape written as Q3_K_S / _M / _L (recipe 11 / 12 /
    13, seed 1), once per session."""
    d = tmp_path_factory.mktemp("q3k_models")
    cache = {}

    def get(preset: int, recipe: int) -> str:
        if (preset, recipe) not in cache:
            cache[preset, recipe] = m.synth_llm_as(str(d / f"llm{preset}_q3k{recipe}.gguf"), preset, recipe, 1)
        return cache[preset, recipe]

    return get


def _silu_mul(g, u):
    g = g.astype(np.float64)
    return g / (1.0 + np.exp(-g)) * u.astype(np.float64)


def _weights(rng, rows, k):
    return m.quantize_rows(11, (rng.standard_normal((rows, k)) * 0.05).astype(np.float32))


# ------------------------------------------------------------------ matvec / matmul kernels
# k: a partial pass (256, 768), one full pass (2048), a pass boundary (2304) and three passes (6144)
@pytest.mark.parametrize("k", [256, 768, 2048, 2304, 6144])
def test_matvec_exact(device, k):
    rng = np.random.default_rng(11000 + k)
    rows = 37
    wq = _weights(rng, rows, k)
    # row 36: the known-answer block in every superblock (codes, high bits and scales that the
    # quantizer never produces together)
    blk, _ = np_q3k.known_answer_block()
    wq[36] = np.tile(blk, k // 256)
    x = rng.standard_normal(k).astype(np.float32)
    x[3] = -9.0
    y = m.debug_matvec(device, 11, wq, k, x)
    ref = np_q3k.dequant(11, wq, rows, k).astype(np.float64) @ np_ref.act_q8_k(x)
    err = np.abs(y - ref)
    print(f"k {k}: max err {err.max():.3g} (known-answer row {err[36]:.3g}), max|y| {np.abs(ref).max():.3g}")
    assert err.max() <= 2e-5 * np.abs(ref).max() + 1e-6
    # the known-answer row's values are ~1e3 times the others': the quantized rows on their own
    assert err[:36].max() <= 2e-5 * np.abs(ref[:36]).max() + 1e-6


@pytest.mark.parametrize("k", [256, 2048])
def test_ceiling_block(device, k):
    """Every code -4, every scale -32, every activation code -127: each 16-group dot is 8128, times
    32 is 260 096 per group and 4 161 536 per superblock, the largest the integer path sees."""
    rows = 9
    wq = np.tile(np_q3k.ceiling_block(), (rows, k // 256))
    x = np.full(k, 1.5, np.float32)
    a = np_ref.act_q8_k(x)
    assert np.allclose(a, 1.5)  # codes -127 times d = -1.5 / 127
    y = m.debug_matvec(device, 11, wq, k, x)
    ref = np_q3k.dequant(11, wq, rows, k).astype(np.float64) @ a
    err = np.abs(y - ref)
    print(f"k {k}: y {y[0]:.9g}, ref {ref[0]:.9g}, max err {err.max():.3g}")
    assert np.all(ref > 0) and err.max() <= 2e-5 * np.abs(ref).max() + 1e-6


@pytest.mark.parametrize("k", [256, 768, 2048, 2304, 6144])
def test_matvec_swiglu_row_pairs(device, k):
    rng = np.random.default_rng(11500 + k)
    rows = 37
    wg, wu = _weights(rng, rows, k), _weights(rng, rows, k)
    x = rng.standard_normal(k).astype(np.float32)
    x[3] = -9.0
    y = m.debug_matvec_swiglu(device, 11, wg, wu, k, x)
    want = _silu_mul(m.debug_matvec(device, 11, wg, k, x), m.debug_matvec(device, 11, wu, k, x))
    err = float(np.abs(y - want).max())
    print(f"k {k}: max err {err:.3g}, max|want| {np.abs(want).max():.3g}")
    assert err <= 1e-5 * float(np.abs(want).max()) + 1e-6


# the last shape has more 16-row tiles than the chip has CUs: the tile-walking kernel
@pytest.mark.parametrize("k,rows,nt", [(256, 50, 3), (2048, 70, 8), (2048, 70, 32), (6144, 33, 16), (2048, 4200, 6)])
def test_mmq_equals_single_token_matvec(device, k, rows, nt):
    rng = np.random.default_rng(11 * 7 + k + nt)
    wq = _weights(rng, rows, k)
    x = rng.standard_normal((nt, k)).astype(np.float32)
    x[:, 3] = -9.0
    y0 = m.debug_mmq(device, 11, wq, k, x)
    refs = [m.debug_matvec(device, 11, wq, k, x[t]) for t in range(nt)]
    for t in range(nt):
        assert np.array_equal(y0[t], refs[t]), (t, float(np.abs(y0[t] - refs[t]).max()))
    r0 = rng.standard_normal((nt, rows)).astype(np.float32)
    y = m.debug_mmq(device, 11, wq, k, x, mode=1, y_in=r0)
    for t in range(nt):
        assert np.array_equal(y[t], refs[t] + r0[t]), t
    wu = _weights(rng, rows, k)
    u0 = m.debug_mmq(device, 11, wu, k, x)
    y = m.debug_mmq(device, 11, wq, k, x, mode=2, up_rows=wu)
    for t in range(nt):
        want = _silu_mul(y0[t], u0[t])
        err = float(np.abs(y[t] - want).max())
        assert err <= 1e-5 * float(np.abs(want).max()) + 1e-6, (t, err)


@pytest.mark.parametrize("nt", [3, 20])
def test_mmq_hand_built_rows(device, nt):
    """The known-answer block and the ceiling block as rows, the all -127 activation as a token: the
    16-row and the 32-row tiles equal the matvec bit for bit at the integer ceilings too."""
    k, rows = 2048, 18
    rng = np.random.default_rng(1111 + nt)
    wq = _weights(rng, rows, k)
    wq[rows - 1] = np.tile(np_q3k.known_answer_block()[0], k // 256)
    wq[rows - 2] = np.tile(np_q3k.ceiling_block(), k // 256)
    x = rng.standard_normal((nt, k)).astype(np.float32)
    x[nt - 1] = 1.5
    y = m.debug_mmq(device, 11, wq, k, x)
    for t in range(nt):
        ref = m.debug_matvec(device, 11, wq, k, x[t])
        assert np.array_equal(y[t], ref), (t, float(np.abs(y[t] - ref).max()))


# ------------------------------------------------------------------ models
POSITIONS = (0, 5, 63, 64, 65, 129)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


# (13, 12) qwen3 as Q3_K_M: both attn_v partners; (14, 11) untied llama as Q3_K_S: a Q3_K embedding;
# (8, 12) lfm2; (17, 13) the 1.7B head shape (hd 128, G 2) as Q3_K_L
@pytest.mark.parametrize("preset,recipe", [(13, 12), (14, 11), (8, 12), (17, 13)])
def test_layers_match_numpy_on_gpu_inputs(device, q3k_path, monkeypatch, preset, recipe):
    """test_q5k_gpu.py::test_layers_match_numpy_on_gpu_inputs's scheme with np_q3k.Mat: each layer
    gets the GPU's layer input and the GPU's K/V rows of the positions before (lfm2 short conv: the
    ring rows of P - 1, P - 2)."""
    monkeypatch.setattr(np_ref, "Mat", np_q3k.Mat)
    path = q3k_path(preset, recipe)
    g = m.Llm(device, path, 256)
    ref = np_ref.DecodeStep(path, POSITIONS[-1] + 8)
    rng = np.random.default_rng(1100 + preset)
    toks = [256, 257] + [int(t) for t in rng.integers(m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800, POSITIONS[-1])]
    errs = []
    for pos in range(POSITIONS[-1] + 1):
        if pos not in POSITIONS:
            g.eval(toks[pos], pos)
            continue
        xs, _ = g.eval_layers(toks[pos], pos)
        assert np.array_equal(xs[0], ref.embed(toks[pos]))  # preset 14: a Q3_K embedding row
        for il in range(g.n_layer):
            if ref.L[il]["conv"] is not None:
                ring = g.conv_ring(il)
                for p in (pos - 1, pos - 2):
                    if p >= 0:
                        ref.bx[il, p] = ring[p & 3]
            elif pos:
                k, v = g.kv_rows(il, pos)
                ref.kc[il, :, :pos] = k
                ref.vc[il, :, :pos] = v
            errs.append((_rel(xs[il + 1], ref.layer(il, xs[il], pos)), pos, il))
    g.close()
    e = np.array([x[0] for x in errs])
    worst = max(errs)
    by_layer, by_pos = {}, {}
    for v, pos, il in errs:
        by_layer.setdefault(il, []).append(v)
        by_pos.setdefault(pos, []).append(v)
    worst_layer = max((np.median(v), il) for il, v in by_layer.items())
    worst_pos = max((np.median(v), pos) for pos, v in by_pos.items())
    print(f"preset {preset} recipe {recipe}: {len(e)} layer evaluations, median {np.median(e):.3g}, max "
          f"{worst[0]:.3g} (pos {worst[1]}, layer {worst[2]}), > 1e-4: {(e > 1e-4).sum()}, worst per-layer median "
          f"{worst_layer[0]:.3g} (layer {worst_layer[1]}), worst per-position median {worst_pos[0]:.3g} "
          f"(pos {worst_pos[1]})")
    assert worst_layer[0] <= 1e-5 and worst_pos[0] <= 1e-5, (worst_layer, worst_pos)
    assert (e > 1e-4).sum() <= 0.12 * len(e)
    assert worst[0] <= 5e-2, worst


@pytest.mark.parametrize("preset,recipe,n", [(13, 12, 2), (13, 12, 40), (13, 12, 150), (14, 11, 17)])
def test_batched_prefill_matches_sequential(device, q3k_path, preset, recipe, n):
    g = m.Llm(device, q3k_path(preset, recipe), 256)
    toks = np.random.default_rng(110 + n).integers(0, g.n_vocab, n)
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
def test_batch_equals_single_streams(device, q3k_path, B):
    g = m.Llm(device, q3k_path(13, 12), 256)
    prompts = _prompts(B, 110 + B)
    seeds = [1100 + 17 * b for b in range(B)]
    got = g.generate_batch(prompts, 24, 0.8, seeds, allow=ALLOW)
    for b in range(B):
        ref = g.generate(prompts[b], 24, 0.8, seeds[b], allow=ALLOW)
        assert np.array_equal(got[b], ref), (b, got[b], ref)
    g.close()


# ------------------------------------------------------------------ the 1.7B shape
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


@pytest.fixture(scope="module")
def preset3_structure(device, synth_llm_path):
    """(step_kinds, batch_step_launches(4)) of preset 3, the 1.7B shape as Q4_K_M."""
    g3 = m.Llm(device, synth_llm_path(3), 256)
    out = (g3.step_kinds(), g3.batch_step_launches(4))
    g3.close()
    return out


def _structure(device, path, preset3_structure):
    kinds3, launches3 = preset3_structure
    g = m.Llm(device, path, 256)
    kinds, launches = g.step_kinds(), g.batch_step_launches(4)
    print(f"kinds 11 / 12: {kinds.count(11)} / {kinds.count(12)} (Q4_K_M {kinds3.count(11)} / {kinds3.count(12)}), "
          f"{len(kinds)} launches per step (Q4_K_M {len(kinds3)}); batched step of 4: {launches} (Q4_K_M {launches3})")
    assert kinds.count(11) == kinds3.count(11) > 0 and kinds.count(12) == kinds3.count(12) > 0
    assert len(kinds) == len(kinds3)
    assert launches == launches3 > 0
    return g, kinds


def test_fused_launches_1p7b_q3km(device, q3k_path, preset3_structure, tmp_path):
    """The 1.7B shape as Q3_K_M (attn_v Q5_K on two layers and Q4_K after, O Q4_K, down Q5_K on
    layer 0 and Q4_K after) runs the attention block and the FFN pair as one launch each on as many
    layers as preset 3 (Q4_K_M) does, and its batched step issues as many launches; a 68-token
    prefill and a 4-stream batched decode (the q|k|v and gate|up launches quantizing in the
    launch, the gate|up tile walk) equal the single-token decode; the fused launches are
    bit-identical with the separate ones."""
    path = q3k_path(3, 12)
    g, kinds = _structure(device, path, preset3_structure)
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


def test_fused_launches_1p7b_q3ks(device, q3k_path, preset3_structure, tmp_path):
    """Q3_K_S: every layer matrix Q3_K (the O, the three-pass down and the v of the fused launches)."""
    path = q3k_path(3, 11)
    g, kinds = _structure(device, path, preset3_structure)
    g.close()
    assert _fused_vs_separate(path, tmp_path) == (kinds.count(11), kinds.count(12))


def test_1p7b_q3kl_loads(device, q3k_path, preset3_structure):
    """Q3_K_L (attn_v, O and down Q5_K) loads with preset 3's launch structure."""
    g, _ = _structure(device, q3k_path(3, 13), preset3_structure)
    g.close()


# ------------------------------------------------------------------ CLI
def _run(args, timeout=300):
    p = subprocess.run([os.path.join(BIN, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"{args[0]} rc={p.returncode}\n{p.stdout}\n{p.stderr[-2000:]}"
    assert "batched decode unavailable" not in p.stderr, p.stderr[-2000:]
    return p.stdout


def test_miotts_batch_equals_single_runs(q3k_path, tmp_path):
    """tests/test_cli_gpu.py's `miotts --batch` check on a Q3_K_M model with the tiny codec."""
    d = tmp_path
    codec = m.synth_codec(str(d / "codec_tiny.gguf"), 1, 1)
    voice = m.synth_voice(str(d / "voice.emb.gguf"), 7)
    prompts = ["テストです。", "こんにちは。", "今日はいい天気ですね。"]
    (d / "batch.txt").write_text("\n".join(prompts) + "\n", "utf-8")
    common = ["-m", q3k_path(13, 12), "-c", codec, "-v", voice, "--max-tokens", 40, "--speech-only", "--ignore-eos"]
    _run(["miotts"] + common + ["--batch", d / "batch.txt", "-o", d / "b.wav", "--gpus", 1])
    for i, p in enumerate(prompts):
        _run(["miotts"] + common + ["-p", p, "-o", d / f"s{i}.wav"])
        assert (d / f"b_{i:03d}.wav").read_bytes() == (d / f"s{i}.wav").read_bytes(), i


# ------------------------------------------------------------------ what stays refused
def _retype(src, dst, name, new_type):
    """Copy GGUF src to dst with tensor `name` declared as ggml type new_type (data kept)."""
    r = gguf_np.GGUFReader(src)
    s = lambda x: struct.pack("<Q", len(x.encode())) + x.encode()
    kvs = [s(k) + raw for k, raw in r.kv_raw]
    align = int(r.kv.get("general.alignment", 32))
    infos, datas, off = [], [], 0
    for t in r.tensors:
        data = bytes(t.raw())
        infos.append(s(t.name) + struct.pack("<I", len(t.ne)) + b"".join(struct.pack("<Q", n) for n in t.ne)
                     + struct.pack("<IQ", new_type if t.name == name else t.type, off))
        datas.append(data)
        off = (off + len(data) + align - 1) // align * align
    head = b"GGUF" + struct.pack("<IQQ", 3, len(infos), len(kvs)) + b"".join(kvs) + b"".join(infos)
    with open(dst, "wb") as f:
        f.write(head)
        f.write(b"\0" * ((len(head) + align - 1) // align * align - len(head)))
        for d in datas:
            f.write(d)
            f.write(b"\0" * ((len(d) + align - 1) // align * align - len(d)))


@pytest.mark.parametrize("new_type,name", [(20, "iq4_nl"), (10, "q2_K")])
def test_iq4_nl_and_q2_k_stay_refused(device, q3k_path, tmp_path, new_type, name):
    """llama-quantize's Q3_K fallback for rows that are not whole superblocks is IQ4_NL (type 20);
    Q2_K (type 10) is the K-quant below: such files fail to load, by the tensor's name and type."""
    dst = str(tmp_path / "x.gguf")
    _retype(q3k_path(13, 12), dst, "blk.1.ffn_up.weight", new_type)
    with pytest.raises(m.HipError, match=rf"blk\.1\.ffn_up\.weight.*(type {new_type}|{name})"):
        m.Llm(device, dst, 64)


def test_q3k_output_matrix_stays_refused(device, q3k_path, tmp_path):
    """llama-quantize's files carry Q6_K as the output matrix; no lm_head kernel exists for type 11."""
    dst = str(tmp_path / "o.gguf")
    _retype(q3k_path(14, 11), dst, "output.weight", 11)
    with pytest.raises(m.HipError, match=r"output\.weight.*(type 11|q3_K)"):
        m.Llm(device, dst, 64)


def test_q3k_embedding_needs_a_q3k_layer_0(device, synth_llm_path, tmp_path):
    """A Q3_K token_embd's row lookup is built into the launches of a Q3_K model only: beside a
    layer 0 of another type (preset 14, Q5_K_S: untied, attn_q Q5_K) the load is refused by the
    tensor's name and type, not run through another type's lookup."""
    dst = str(tmp_path / "e.gguf")
    _retype(synth_llm_path(14), dst, "token_embd.weight", 11)
    with pytest.raises(m.HipError, match=r"token_embd\.weight.*q3_K.*layer 0"):
        m.Llm(device, dst, 64)
