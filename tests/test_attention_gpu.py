"""GPU parity: the decode step's attention launches (k_attention, k_att_o; csrc/hip/llm_attention.h,
attend_chunk_mfma / merge_out4 / attn_merge_last in csrc/hip/llm_device.h) against the float64
attention of tests/np_attn.py, on injected K/V states up to n_ctx 32768.

One launch per case (mio_hip_llm_debug_attention) on a raw q|k|v row and a cache written with
mio_hip_llm_set_kv_rows; the output compared is LlmBuffers.att itself. Head shapes: (hd 64, G 2)
qwen2 with q/k/v biases, (64, 3) qwen3, (128, 2) qwen3 with non-trivial q/k norm weights, (64, 4)
llama (NORM RoPE pairing): the last three have the attention + O launch (which = 10), all have
the attention launch (which = 1). Positions np_attn.POSITIONS, patterns np_attn.PATTERNS (Cases).
The raw rows are nudged (np_attn.Model.nudge) so no prepared element sits beside an f16 rounding
midpoint: the K/V row the launch appends at `pos` must equal the reference's BIT FOR BIT, and no
comparison here has an allowance for flipped roundings.

Error model (u = 2^-24; one head, cached + new rows t = 0..pos, scores s_t, softmax weights
w_t = p_t / L, M = max s, nb = merge batches of 8 chunks of 64 positions):

  * score: hd exact f16 x f16 products accumulated in f32 by the MFMA, worst case sequential:
    |ds_t| <= u (hd A_t + 2 |s_t|), A_t = sum_i |q_i k_ti| / sqrt(hd) (the 2 |s_t|: the f32
    scale and its product). A score error is a relative error of the weight (e^ds - 1);
  * exponent chain: the weight of position t is a product of exp(s_t - M_chunk) (v_exp_f32 of
    (s - M) log2 e: argument rounding 3 u |s - M|, the instruction |x| 2^-24 + 1 ulp, x = 1.44
    (s - M)), expf(M_chunk - M_batch) and expf(M_batch - M_later) per later batch whose max is
    larger; the arguments are non-negative and sum to M - s_t, so together
    <= 4.5 u (M - s_t) + 2 u (nb + 2);
  * P as f16 hi + lo for the P.V MFMA: residue 2^-22 p_t, or, where p_t (relative to its chunk's
    max) is below 2^-14 and hi / lo are f16 subnormals, at most min(p_t, 2^-25) absolute:
    a_t = min(w_t, 2^-25 e^(M_chunk - M) / L);
  * f32 sums: 64 positions per chunk in the P.V MFMA and in l, then per merge batch one rescale
    and 8 multiply-adds, and the final division: gamma = (64 + 10 nb + 4) u of sum_t w_t |v_t|.

  E_t = u (hd A_t + 2 |s_t|) + 4.5 u (M - s_t) + 2 u (nb + 2) + 2^-22 is the relative error of
  weight t before normalization. Normalizing cancels the part common to all weights: with
  Ebar = sum_t w_t E_t, |w'_t - w_t| <= w_t (E_t (1 - 2 w_t) + Ebar) (zero for a single dominant
  weight). Each output d is bounded by

      4 [ sum_t w_t (E_t (1 - 2 w_t) + Ebar) |v_td| + 2 gamma sum_t w_t |v_td| + sum_t a_t |v_td| ]
      + 2^-95 max |v|

  the bracket being the model times sum_t p_t |v_t| / L with the model inside the sum, 4 the
  margin for summation order, and the last term p_t flushed below 2^-126 (times 2^15 positions
  and |v| <= 2^16). np_attn.bound computes it; tests/test_attention_ref.py shows that it is
  tight enough to catch a dropped or doubled position, a neighbour's RoPE row, P without its low
  part, a missing rescale and a skipped chunk.

Poison: rows pos .. end of the last chunk of the cache (row pos is the one kv_issue reads for
the masked rows; the launch writes it) are filled with f16 NaN, then Inf, before the call: the
output must be the bits of the same call with those rows zero.

Measured on the MI355X, worst err / bound per pattern over every shape, launch and position
(which = 1 and which = 10 give the same bits):

  census 0.0064   flat 0.0031   flat_census 0.0074   peaked8 0.051   peaked40 0.125
  dominant 0 (the output is the dominant V row exactly)   far_apart 0.00022   range 0.0020
  vsubnormal 0.0055 (the P.V MFMA keeps f16-subnormal values: no floor)   poison 0.0031

The errors are far inside the bound because the model takes every f32 sum at its sequential
worst case (hd u for a score, 64 u for a chunk) where the hardware sums in trees; the mutants of
tests/test_attention_ref.py are the measure of what the bound still catches.
Poison, before the fix in kv_issue (csrc/hip/llm_device.h): every output of every head NaN at
pos 0 for all four shapes, both launches; with the V (and K) rows loaded by range-checked buffer
loads over the written rows, the outputs are the zero-filled call's bits.
"""
import numpy as np
import pytest

import miotts_amd as m
import np_attn as A

pytestmark = pytest.mark.gpu

SHAPES = {5: (1,), 9: (1, 10), 17: (1, 10), 18: (1, 10)}
CASES = [(p, pat, w) for p, ws in SHAPES.items() for pat in A.PATTERNS for w in ws]

_models = {}
_runs = {}  # the reference of the last (preset, pattern): shared by its launches


@pytest.fixture(scope="module")
def models(device, synth_llm_path):
    def get(preset):
        if preset not in _models:
            path = synth_llm_path(preset)
            _models[preset] = (m.Llm(device, path, A.N_CTX), A.Cases(A.Model(path)))
        return _models[preset]

    yield get
    for g, _ in _models.values():
        g.close()
    _models.clear()
    _runs.clear()


def _reference(C, preset, pattern):
    """[(pos, label, edit, raw, k16, v16, out [H, hd], bound [H, hd])] and the f16 state."""
    key = (preset, pattern)
    if key in _runs:
        return _runs[key]
    _runs.clear()
    mod = C.m
    H, Hk, G = mod.n_head, mod.n_kv, mod.G
    K16, V16 = C.state(pattern)
    K, V = K16.astype(np.float64), V16.astype(np.float64)
    runs = []
    for pos in A.POSITIONS:
        raw = C.raw(pos, census=pattern == "census")
        q, k, v = mod.prepare(0, raw, pos)
        for label, edit in C.edits(pattern, pos):
            rows = [t for t, _, _ in edit] + [pos]
            for t, kr, vr in edit:
                K[:, t], V[:, t] = kr, vr
            K[:, pos], V[:, pos] = k, v
            out, bnd = np.empty((H, mod.hd)), np.empty((H, mod.hd))
            for h in range(H):
                Kh, Vh = K[h // G, :pos + 1], V[h // G, :pos + 1]
                out[h], s, w = A.attend(q[h], Kh, Vh)
                bnd[h] = A.bound(q[h], Kh, Vh, s, w)
            K[:, rows], V[:, rows] = K16[:, rows], V16[:, rows]
            runs.append((pos, label, edit, raw, k, v, out, bnd))
    _runs[key] = (K16, V16, runs)
    return _runs[key]


def _put(g, K16, V16, lo, hi):
    g.set_kv_rows(0, lo, K16[:, lo:hi], V16[:, lo:hi])


@pytest.mark.parametrize("preset,pattern,which", CASES)
def test_attention_against_float64(models, preset, pattern, which):
    g, C = models(preset)
    K16, V16, runs = _reference(C, preset, pattern)
    _put(g, K16, V16, 0, A.N_CTX)
    worst = (0.0, None)
    for pos, label, edit, raw, k, v, out, bnd in runs:
        for t, kr, vr in edit:
            g.set_kv_rows(0, t, kr[:, None, :], vr[:, None, :])
        end = min(A.CHUNK * (pos // A.CHUNK + 1), A.N_CTX)
        if pattern == "poison":
            outs = {}
            for name, bits in (("zero", 0x0000), ("nan", 0x7E00), ("inf", 0x7C00), ("-inf", 0xFC00)):
                fill = np.full((C.m.n_kv, end - pos, C.m.hd), bits, np.uint16).view(np.float16)
                g.set_kv_rows(0, pos, fill, fill)
                outs[name] = g.debug_attention(0, pos, which, raw)
            att = outs["zero"]
            for name in ("nan", "inf", "-inf"):
                assert outs[name].tobytes() == att.tobytes(), (pos, name, int(np.isnan(outs[name]).sum()))
        else:
            att = g.debug_attention(0, pos, which, raw)
        kg, vg = g.kv_rows(0, pos + 1)
        assert np.array_equal(kg[:, pos].view(np.uint16), k.view(np.uint16)), (pos, label)
        assert np.array_equal(vg[:, pos].view(np.uint16), v.view(np.uint16)), (pos, label)
        assert np.isfinite(att).all(), (pos, label)
        ratio = np.abs(att - out) / bnd
        if ratio.max() > worst[0]:
            worst = (float(ratio.max()), (pos, label))
        assert ratio.max() <= 1.0, (pos, label, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
        for t in sorted({t for t, _, _ in edit}):
            _put(g, K16, V16, t, t + 1)
        _put(g, K16, V16, pos, end)
    print(f"attention preset {preset} {pattern} which={which}: worst err/bound {worst[0]:.3g} at {worst[1]}")


def test_entry_points_refuse_what_they_cannot_run(device, models, synth_llm_path):
    g, C = models(5)  # (hd 64, G 2): no attention + O launch
    raw = C.raw(3)
    for which in (10, 0, 2, 11):
        with pytest.raises(m.HipError, match="rc=-6"):
            g.debug_attention(0, 3, which, raw)
    with pytest.raises(m.HipError, match="rc=-1"):
        g.debug_attention(0, A.N_CTX, 1, raw)
    with pytest.raises(m.HipError, match="rc=-1"):
        g.debug_attention(g.n_layer, 3, 1, raw)
    k = np.zeros((g.n_kv, 2, g.head_dim), np.float16)
    with pytest.raises(m.HipError, match="rc=-1"):
        g.set_kv_rows(0, A.N_CTX - 1, k, k)
    lf = m.Llm(device, synth_llm_path(7), 64)  # tiny lfm2: layer 0 is a short-conv layer
    with pytest.raises(m.HipError, match="rc=-1"):
        lf.debug_attention(0, 3, 1, np.zeros((lf.n_head + 2 * lf.n_kv) * lf.head_dim, np.float32))
    lf.close()


def test_set_kv_rows_is_the_inverse_of_kv_rows(models):
    g, _ = models(18)
    rng = np.random.default_rng(5)
    k = rng.integers(0, 0x7C00, (g.n_kv, 70, g.head_dim)).astype(np.uint16).view(np.float16)
    v = rng.integers(0, 0x7C00, (g.n_kv, 70, g.head_dim)).astype(np.uint16).view(np.float16)
    for il in range(g.n_layer):
        g.set_kv_rows(il, 100 + il, k, v)
    for il in range(g.n_layer):
        kg, vg = g.kv_rows(il, 170 + il)
        assert np.array_equal(kg[:, 100 + il:].view(np.uint16), k.view(np.uint16))
        assert np.array_equal(vg[:, 100 + il:].view(np.uint16), v.view(np.uint16))
