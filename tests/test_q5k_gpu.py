"""GPU parity: Q5_K weights (ggml type 13; Q5_K_M / Q5_K_S files) on every LLM path.

The C oracle does not read type 13, so the reference is tests/np_q5k.py (an independent numpy
restatement of the block format) swapped into np_ref.DecodeStep.

 * matvec: the GPU's per-superblock integer sums are exact and only the float sum over
   superblocks is reordered, so against the float64 dequant(w) @ act_q8_k(x) the project's bound
   of test_llm_gpu.py holds: 2e-5 * max|y| + 1e-6;
 * the int8-MFMA matmul, the batched prefill and the batched decode equal the single-token
   decode BIT FOR BIT (same integer sums, same float terms, same lane / tree order);
 * layer by layer against the numpy layer on the GPU's own layer input and K/V rows (conv ring
   for lfm2): the derived bounds of test_llm_layers_gpu.py (the two differ in float summation
   order only, so ~1e-6 unless a last-ulp difference re-rounds a Q8_K block or an f16 value);
 * the fused launches (attention block, FFN pair) exist for the 1.7B Q5_K_M shapes and are
   bit-identical with the separate launches.
"""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import miotts_amd as m
import np_q5k
import np_ref
from miotts_amd import gguf_np

pytestmark = pytest.mark.gpu

ALLOW = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800)


# ------------------------------------------------------------------ matvec / matmul kernels
# k: a partial pass (256, 768), one full pass (2048), a pass boundary (2304) and three passes (6144)
@pytest.mark.parametrize("k", [256, 768, 2048, 2304, 6144])
def test_matvec_exact(device, k):
    rng = np.random.default_rng(13000 + k)
    rows = 37
    w = (rng.standard_normal((rows, k)) * 0.05).astype(np.float32)
    wq = m.quantize_rows(13, w)
    # row 36: the known-answer block in every superblock (codes, scales and fifth bits that the
    # quantizer never produces together)
    blk, _ = np_q5k.known_answer_block()
    wq[36] = np.tile(blk, k // 256)
    x = rng.standard_normal(k).astype(np.float32)
    x[3] = -9.0
    y = m.debug_matvec(device, 13, wq, k, x)
    ref = np_q5k.dequant(13, wq, rows, k).astype(np.float64) @ np_ref.act_q8_k(x)
    err = np.abs(y - ref)
    print(f"k {k}: max err {err.max():.3g} (known-answer row {err[36]:.3g}), max|y| {np.abs(ref).max():.3g}")
    assert err.max() <= 2e-5 * np.abs(ref).max() + 1e-6
    # the known-answer row's values are ~1e4 times the others': the quantized rows on their own
    assert err[:36].max() <= 2e-5 * np.abs(ref[:36]).max() + 1e-6


# the last shape has more 16-row tiles than the chip has CUs: the tile-walking kernel
@pytest.mark.parametrize("k,rows,nt", [(256, 50, 3), (2048, 70, 8), (2048, 70, 32), (6144, 33, 16), (6144, 32, 40),
                                       (2048, 4200, 6)])
def test_mmq_equals_single_token_matvec(device, k, rows, nt):
    """The modes of test_llm_gpu.py::test_mmq_equals_single_token_matvec for type 13."""
    rng = np.random.default_rng(13 * 7 + k + nt)
    w = (rng.standard_normal((rows, k)) * 0.05).astype(np.float32)
    wq = m.quantize_rows(13, w)
    x = rng.standard_normal((nt, k)).astype(np.float32)
    x[:, 3] = -9.0
    y = m.debug_mmq(device, 13, wq, k, x)
    refs = [m.debug_matvec(device, 13, wq, k, x[t]) for t in range(nt)]
    for t in range(nt):
        assert np.array_equal(y[t], refs[t]), (t, float(np.abs(y[t] - refs[t]).max()))
    r0 = rng.standard_normal((nt, rows)).astype(np.float32)
    y = m.debug_mmq(device, 13, wq, k, x, mode=1, y_in=r0)
    for t in range(nt):
        assert np.array_equal(y[t], refs[t] + r0[t]), t
    wu = m.quantize_rows(13, (rng.standard_normal((rows, k)) * 0.05).astype(np.float32))
    y = m.debug_mmq(device, 13, wq, k, x, mode=2, up_rows=wu)
    for t in range(nt):
        # expf differs from numpy's exp by an ulp (the model-level tests below pin this epilogue
        # bit-exactly against the decode step)
        u = m.debug_matvec(device, 13, wu, k, x[t])
        g = refs[t].astype(np.float64)
        want = g / (1.0 + np.exp(-g)) * u
        err = float(np.abs(y[t] - want).max())
        assert err <= 1e-5 * float(np.abs(want).max()) + 1e-6, (t, err)


# ------------------------------------------------------------------ models
POSITIONS = (0, 5, 63, 64, 65, 129)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


@pytest.mark.parametrize("preset", [13, 14, 15])
def test_layers_match_numpy_on_gpu_inputs(device, synth_llm_path, monkeypatch, preset):
    """test_llm_layers_gpu.py's scheme with np_ref.DecodeStep (Q5_K through np_q5k.Mat) as the
    reference: each layer gets the GPU's layer input and the GPU's K/V rows of the positions
    before (lfm2 short conv: the ring rows of P - 1, P - 2)."""
    monkeypatch.setattr(np_ref, "Mat", np_q5k.Mat)
    path = synth_llm_path(preset)
    g = m.Llm(device, path, 256)
    ref = np_ref.DecodeStep(path, POSITIONS[-1] + 8)
    rng = np.random.default_rng(1300 + preset)
    toks = [256, 257] + [int(t) for t in rng.integers(m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800, POSITIONS[-1])]
    errs = []
    for pos in range(POSITIONS[-1] + 1):
        if pos not in POSITIONS:
            g.eval(toks[pos], pos)
            continue
        xs, _ = g.eval_layers(toks[pos], pos)
        assert np.array_equal(xs[0], ref.embed(toks[pos]))  # preset 14: a Q5_K embedding row
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
    print(f"preset {preset}: {len(e)} layer evaluations, median {np.median(e):.3g}, max {worst[0]:.3g} "
          f"(pos {worst[1]}, layer {worst[2]}), > 1e-4: {(e > 1e-4).sum()}, worst per-layer median "
          f"{worst_layer[0]:.3g} (layer {worst_layer[1]}), worst per-position median {worst_pos[0]:.3g} "
          f"(pos {worst_pos[1]})")
    assert worst_layer[0] <= 1e-5 and worst_pos[0] <= 1e-5, (worst_layer, worst_pos)
    assert (e > 1e-4).sum() <= 0.12 * len(e)
    assert worst[0] <= 5e-2, worst


@pytest.mark.parametrize("preset,n", [(13, 2), (13, 40), (13, 150), (14, 17)])
def test_batched_prefill_matches_sequential(device, synth_llm_path, preset, n):
    g = m.Llm(device, synth_llm_path(preset), 256)
    toks = np.random.default_rng(130 + n).integers(0, g.n_vocab, n)
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
def test_batch_equals_single_streams(device, synth_llm_path, B):
    g = m.Llm(device, synth_llm_path(13), 256)
    prompts = _prompts(B, 130 + B)
    seeds = [1300 + 17 * b for b in range(B)]
    got = g.generate_batch(prompts, 24, 0.8, seeds, allow=ALLOW)
    for b in range(B):
        ref = g.generate(prompts[b], 24, 0.8, seeds[b], allow=ALLOW)
        assert np.array_equal(got[b], ref), (b, got[b], ref)
    g.close()


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


def test_fused_launches_1p7b_q5km(device, synth_llm_path, tmp_path):
    """Preset 16 (the 1.7B shape as Q5_K_M) runs the attention block and the FFN pair as one
    launch each on as many layers as preset 3 (Q4_K_M) does, bit-identical with the separate
    launches (a fresh process per variant: the switches are read once); a 68-token prefill and a
    4-stream batched decode (the fused gate|up walk and the three-pass down of the 16-token
    tiles) equal the single-token decode."""
    path = synth_llm_path(16)
    g = m.Llm(device, path, 256)
    kinds = g.step_kinds()
    g3 = m.Llm(device, synth_llm_path(3), 256)
    kinds3 = g3.step_kinds()
    g3.close()
    assert kinds.count(11) == kinds3.count(11) > 0 and kinds.count(12) == kinds3.count(12) > 0
    toks = np.random.default_rng(68).integers(0, 151936, 68)
    batched = g.prefill(toks)
    for pos, t in enumerate(toks):
        seq = g.eval(int(t), pos)
    assert np.array_equal(batched, seq), float(np.abs(batched - seq).max())
    prompts = _prompts(4, 16)
    got = g.generate_batch(prompts, 12, 0.8, [42, 43, 44, 45], allow=ALLOW)
    for b in range(4):
        assert np.array_equal(got[b], g.generate(prompts[b], 12, 0.8, 42 + b, allow=ALLOW)), b
    g.close()
    script = tmp_path / "fusion.py"
    script.write_text(_FUSION_SCRIPT)
    pkg = os.path.dirname(os.path.dirname(m.__file__))
    outs = {}
    for name, env in (("fused", {}), ("separate", {"MIO_LAYER_ATT": "0", "MIO_ATT_FUSE_O": "0", "MIO_FFN_FUSE": "0"})):
        p = subprocess.run([sys.executable, str(script), path, pkg], capture_output=True, text=True, timeout=240,
                           env=dict(os.environ, **env))
        assert p.returncode == 0, p.stderr[-2000:]
        outs[name] = p.stdout.split()
    print(outs)
    assert int(outs["fused"][0]) == kinds.count(11) and int(outs["fused"][1]) == kinds.count(12)
    assert int(outs["separate"][0]) == 0 and int(outs["separate"][1]) == 0
    assert int(outs["fused"][2]) == 40
    assert outs["fused"][3] == outs["separate"][3], outs


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


def test_q5_1_stays_refused(device, synth_llm_path, tmp_path):
    """llama-quantize's Q5_K fallback for rows that are not whole superblocks is Q5_1 (type 7):
    such a file fails to load, by the tensor's name and type."""
    dst = str(tmp_path / "q5_1.gguf")
    _retype(synth_llm_path(13), dst, "blk.1.ffn_up.weight", 7)
    with pytest.raises(m.HipError, match=r"blk\.1\.ffn_up\.weight.*(type 7|q5_1)"):
        m.Llm(device, dst, 64)
