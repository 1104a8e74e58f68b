"""GPU parity: IQ4_XS weights (ggml type 23; recipe 23 of the synthetic writer) on every LLM path.

The reference is tests/np_iq4xs.py (a numpy restatement of the block format) swapped into
np_ref.DecodeStep. Bounds, as for the other K-quants (test_q3k_gpu.py states each one's reason; DESIGN.md
"Numerics" derives the layer bounds): matvec 2e-5 * max|y| + 1e-6 against the float64 dequant(w) @
act_q8_k(x), since the per-superblock sums are exact integers and only the float sum over
superblocks is reordered; SwiGLU 1e-5 * max + 1e-6; the int8-MFMA matmul, the prefill and the
batched decode equal the single-token decode bit for bit; fused launches equal separate ones.
"""
import numpy as np
import pytest

import miotts_amd as m
import np_iq4xs
import np_ref
from test_q3k_gpu import ALLOW, POSITIONS, _fused_vs_separate, _prompts, _rel, _silu_mul
from test_q5k_gpu import _retype

pytestmark = pytest.mark.gpu
T = 23
KS = [256, 768, 2048, 2304, 6144]  # a partial pass, a full pass, a pass boundary, three passes


@pytest.fixture(scope="module")
def iq4_path(tmp_path_factory):
    d, cache = tmp_path_factory.mktemp("iq4xs_models"), {}

    def get(preset: int, n_layer: int = 0) -> str:
        if (preset, n_layer) not in cache:
            cache[preset, n_layer] = m.synth_llm_shape(str(d / f"llm{preset}_{n_layer}.gguf"), preset, T, 1, n_layer=n_layer)
        return cache[preset, n_layer]

    return get


def _weights(rng, rows, k):
    return m.quantize_rows(T, (rng.standard_normal((rows, k)) * 0.05).astype(np.float32))


def _x(rng, *shape):
    x = rng.standard_normal(shape).astype(np.float32)
    x[..., 3] = -9.0
    return x


@pytest.mark.parametrize("k", KS)
def test_matvec_exact(device, k):
    rng = np.random.default_rng(23000 + k)
    wq = _weights(rng, 37, k)
    wq[36] = np.tile(np_iq4xs.known_answer_block()[0], k // 256)
    x = _x(rng, k)
    y = m.debug_matvec(device, T, wq, k, x)
    ref = np_iq4xs.dequant(wq, 37, k).astype(np.float64) @ np_ref.act_q8_k(x)
    err = np.abs(y - ref)
    print(f"k {k}: max err {err.max():.3g} (known-answer row {err[36]:.3g}), max|y| {np.abs(ref).max():.3g}")
    assert err.max() <= 2e-5 * np.abs(ref).max() + 1e-6
    assert err[:36].max() <= 2e-5 * np.abs(ref[:36]).max() + 1e-6  # the quantized rows on their own


@pytest.mark.parametrize("k", [256, 2048])
def test_ceiling_block(device, k):
    """Every weight code 0 and scale -32, every activation code -127: |isum| = 132 128 768 per superblock,
    above 2^24, so its conversion to float rounds (relative 2^-25, far inside the bound)."""
    wq = np.tile(np_iq4xs.ceiling_block(), (9, k // 256))
    x = np.full(k, 1.5, np.float32)
    y = m.debug_matvec(device, T, wq, k, x)
    ref = np_iq4xs.dequant(wq, 9, k).astype(np.float64) @ np_ref.act_q8_k(x)
    err = np.abs(y - ref)
    print(f"k {k}: y {y[0]:.9g}, ref {ref[0]:.9g}, max err {err.max():.3g}")
    assert np.all(ref > 0) and err.max() <= 2e-5 * np.abs(ref).max() + 1e-6


@pytest.mark.parametrize("k", KS)
def test_matvec_swiglu_row_pairs(device, k):
    rng = np.random.default_rng(23500 + k)
    wg, wu, x = _weights(rng, 37, k), _weights(rng, 37, k), _x(rng, k)
    y = m.debug_matvec_swiglu(device, T, wg, wu, k, x)
    want = _silu_mul(m.debug_matvec(device, T, wg, k, x), m.debug_matvec(device, T, wu, k, x))
    assert float(np.abs(y - want).max()) <= 1e-5 * float(np.abs(want).max()) + 1e-6


# 16-row tiles (nt <= 16) and 32-row tiles; the last shape has more tiles than CUs: the tile walk
@pytest.mark.parametrize("k,rows,nt", [(256, 50, 3), (2048, 70, 8), (2048, 70, 32), (6144, 33, 16), (2048, 4200, 6)])
def test_mmq_equals_single_token_matvec(device, k, rows, nt):
    rng = np.random.default_rng(23 * 7 + k + nt)
    wq = _weights(rng, rows, k)
    wq[rows - 1] = np.tile(np_iq4xs.known_answer_block()[0], k // 256)
    wq[rows - 2] = np.tile(np_iq4xs.ceiling_block(), k // 256)
    x = _x(rng, nt, k)
    x[nt - 1] = 1.5
    refs = np.stack([m.debug_matvec(device, T, wq, k, x[t]) for t in range(nt)])
    y0 = m.debug_mmq(device, T, wq, k, x)
    assert np.array_equal(y0, refs), float(np.abs(y0 - refs).max())
    r0 = rng.standard_normal((nt, rows)).astype(np.float32)
    assert np.array_equal(m.debug_mmq(device, T, wq, k, x, mode=1, y_in=r0), refs + r0)
    wu = _weights(rng, rows, k)
    with np.errstate(over="ignore"):  # exp(-g) of the ceiling row's g ~ -1e7: silu is -0 there
        want = _silu_mul(y0, m.debug_mmq(device, T, wu, k, x))
    y = m.debug_mmq(device, T, wq, k, x, mode=2, up_rows=wu)
    assert np.all(np.abs(y - want).max(1) <= 1e-5 * np.abs(want).max(1) + 1e-6)


# 13: qwen3, G 2 (v IQ4_XS); 14: untied llama (an IQ4_XS embedding row); 8: lfm2; 18: hd 64, G 4 (v Q5_K);
# 17 with 8 layers: hd 128, G 2, layer 0's down Q5_K
@pytest.mark.parametrize("preset,n_layer", [(13, 0), (14, 0), (8, 0), (18, 0), (17, 8)])
def test_layers_match_numpy_on_gpu_inputs(device, iq4_path, monkeypatch, preset, n_layer):
    """test_q5k_gpu.py::test_layers_match_numpy_on_gpu_inputs's scheme and bounds with np_iq4xs.Mat."""
    monkeypatch.setattr(np_ref, "Mat", np_iq4xs.Mat)
    path = iq4_path(preset, n_layer)
    g = m.Llm(device, path, 256)
    ref = np_ref.DecodeStep(path, POSITIONS[-1] + 8)
    rng = np.random.default_rng(2300 + preset)
    toks = [256, 257] + [int(t) for t in rng.integers(m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800, POSITIONS[-1])]
    errs = []
    for pos in range(POSITIONS[-1] + 1):
        if pos not in POSITIONS:
            g.eval(toks[pos], pos)
            continue
        xs, _ = g.eval_layers(toks[pos], pos)
        assert np.array_equal(xs[0], ref.embed(toks[pos]))
        for il in range(g.n_layer):
            if ref.L[il]["conv"] is not None:
                ring = g.conv_ring(il)
                for p in (pos - 1, pos - 2):
                    if p >= 0:
                        ref.bx[il, p] = ring[p & 3]
            elif pos:
                ref.kc[il, :, :pos], ref.vc[il, :, :pos] = g.kv_rows(il, pos)
            errs.append((_rel(xs[il + 1], ref.layer(il, xs[il], pos)), pos, il))
    g.close()
    e = np.array([x[0] for x in errs])
    med = lambda key: max(np.median([v for v, pos, il in errs if (pos, il)[key] == i]) for i in {x[1 + key] for x in errs})
    print(f"preset {preset}: {len(e)} layer evaluations, median {np.median(e):.3g}, max {max(errs)}, "
          f"> 1e-4: {(e > 1e-4).sum()}, worst per-position / per-layer median {med(0):.3g} / {med(1):.3g}")
    assert med(0) <= 1e-5 and med(1) <= 1e-5
    assert (e > 1e-4).sum() <= 0.12 * len(e) and e.max() <= 5e-2


@pytest.mark.parametrize("preset,n", [(13, 2), (13, 150), (8, 40)])
def test_batched_prefill_matches_sequential(device, iq4_path, preset, n):
    g = m.Llm(device, iq4_path(preset), 256)
    toks = np.random.default_rng(230 + n).integers(0, g.n_vocab, n)
    batched = g.prefill(toks)
    for pos, t in enumerate(toks):
        seq = g.eval(int(t), pos)
    g.close()
    assert np.array_equal(batched, seq), float(np.abs(batched - seq).max())


# B = 3: the launches that quantize their input themselves; B = 9: plain 16-token tiles
@pytest.mark.parametrize("preset,B", [(13, 3), (13, 9), (8, 3)])
def test_batch_equals_single_streams(device, iq4_path, preset, B):
    g = m.Llm(device, iq4_path(preset), 256)
    prompts, seeds = _prompts(B, 230 + B), [2300 + 17 * b for b in range(B)]
    got = g.generate_batch(prompts, 24, 0.8, seeds, allow=ALLOW)
    for b in range(B):
        assert np.array_equal(got[b], g.generate(prompts[b], 24, 0.8, seeds[b], allow=ALLOW)), b
    g.close()


def test_fused_launches_1p7b(device, iq4_path, synth_llm_path, tmp_path):
    """The 1.7B shape as IQ4_XS (v IQ4_XS, down Q5_K on layers 0-2) runs the attention block and the
    FFN pair as one launch each on as many layers as preset 3 (Q4_K_M), bit-identical with the
    separate launches."""
    kinds = []
    for path in (synth_llm_path(3), iq4_path(3)):
        g = m.Llm(device, path, 256)
        kinds.append(g.step_kinds())
        g.close()
    assert len(kinds[1]) == len(kinds[0]) and kinds[1].count(11) == kinds[0].count(11) > 0
    assert kinds[1].count(12) == kinds[0].count(12) > 0
    assert _fused_vs_separate(iq4_path(3), tmp_path) == (kinds[1].count(11), kinds[1].count(12))


def test_refusals(device, iq4_path, synth_llm_path, tmp_path):
    """No lm_head kernel exists for type 23, and an IQ4_XS table's lookup is built into the launches of
    an IQ4_XS model only: both loads fail by the tensor's name and type."""
    dst = str(tmp_path / "x.gguf")
    _retype(iq4_path(14), dst, "output.weight", T)
    with pytest.raises(m.HipError, match=r"output\.weight.*iq4_xs"):
        m.Llm(device, dst, 64)
    _retype(synth_llm_path(14), dst, "token_embd.weight", T)  # preset 14: untied, layer 0 Q5_K
    with pytest.raises(m.HipError, match=r"token_embd\.weight.*iq4_xs.*layer 0"):
        m.Llm(device, dst, 64)
