"""CPU: self-checks of the float64 attention reference (tests/np_attn.py) and the teeth of
tests/test_attention_gpu.py.

Self-checks: the RoPE table row against np_ref's table, the prepared heads against
np_ref.DecodeStep's f32 preparation, the plain softmax against the chunked restatement, the
nudged inputs' margin, the midpoint distance.

Teeth: each mutant below is applied to the float64 reference at a case of the GPU test (same
builders, same bound), and its output must leave the bound there, in at least one output of the
head: a kernel with that defect would fail the GPU test at that case.

  mutant                                   case
  one position dropped at a chunk edge     census, pos 4096 and 32767
  one position counted twice               census, pos 4096 and 32767
  RoPE row pos - 1 / pos + 1               flat at 65 and 4096, peaked8 at 513
  P rounded to f16, no low part            flat_census at 63 (one chunk, each output one p_t)
  accumulators not rescaled between        far_apart at 1023 and 4096
  merge batches
  one whole chunk skipped                  dominant (the chunk of t*), census at 4096

A whole chunk missing from the census at a position that is a multiple of 64 removes one count
from each of hd = 64 dimensions alike and leaves the mean unchanged: the census sees a skipped
chunk at hd 128 (and at 4096 + 1 positions), the dominant and peaked patterns see it at hd 64.
"""
import numpy as np
import pytest

import miotts_amd as m
import np_attn as A
import np_ref

PRESETS = (5, 9, 17, 18)  # (hd 64, G 2, qwen2 biases), (64, 3, qwen3), (128, 2, qwen3), (64, 4, llama)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("attn_ref")
    out = {}
    for p in PRESETS:
        path = m.synth_llm(str(d / f"llm{p}.gguf"), p, 1)
        out[p] = (path, A.Cases(A.Model(path), n_ctx=A.N_CTX if p in (5, 17) else 4352))
    return out


def _head_case(C, pattern, pos, h, edit=None, census=False):
    """(q, K, V, out, bound, raw) of head h for a pattern at pos (edit: rows replaced first)."""
    mod = C.m
    K16, V16 = C.state(pattern)
    kv = h // mod.G
    raw = C.raw(pos, census=census)
    q, k, v = mod.prepare(0, raw, pos)
    K, V = K16[kv, :pos + 1].astype(np.float64), V16[kv, :pos + 1].astype(np.float64)
    for t, kr, vr in edit or []:
        K[t], V[t] = kr[kv], vr[kv]
    K[pos], V[pos] = k[kv], v[kv]
    out, s, w = A.attend(q[h], K, V)
    return q[h].astype(np.float64), K, V, out, A.bound(q[h], K, V, s, w), raw


def _worst(got, want, bnd):
    return float((np.abs(got - want) / bnd).max())


def test_midpoint_distance():
    one = np.float64(np.float16(1.0))
    ulp = 2.0 ** -10
    y = np.array([1.0, 1.0 + 0.5 * ulp - 1e-9, 1.0 + 0.5 * ulp + 1e-9, 1.0 - 0.25 * ulp + 1e-9, 3.0e-8, 0.0])
    want = np.array([0.25 * ulp, 1e-9, 1e-9, 1e-9, abs(3.0e-8 - 2.0 ** -25), 2.0 ** -25])
    assert np.allclose(A.midpoint_distance(y), want, rtol=0, atol=1e-12), A.midpoint_distance(y)
    assert one == 1.0


@pytest.mark.parametrize("preset", PRESETS)
def test_preparation_matches_np_ref(cases, preset):
    """rope_row is np_ref's table row (1 f32 ulp: cos / sin of the same f32 angles), and the f16 q,
    k, v rows are np_ref.DecodeStep's (its f32 preparation) except where a rounding flipped, which
    the nudged rows exclude: bit for bit."""
    path, C = cases[preset]
    mod = C.m
    ref = np_ref.DecodeStep(path, 80)
    for pos in (0, 1, 63, 79):
        c, s = mod.rope_row(pos)
        assert np.abs(ref.rope[pos, :, 0] - c).max() <= 2.0 ** -23 and np.abs(ref.rope[pos, :, 1] - s).max() <= 2.0 ** -23
        raw = C.raw(pos)
        assert not any(a.any() for a in mod.ambiguous(0, raw, pos))
        q, k, v = mod.prepare(0, raw, pos)
        L, H, Hk, hd = ref.L[0], mod.n_head, mod.n_kv, mod.hd
        rq, rk, rv = raw[:H * hd], raw[H * hd:(H + Hk) * hd], raw[(H + Hk) * hd:]
        if L["bq"] is not None:
            rq, rk, rv = (rq + L["bq"]).astype(np.float32), (rk + L["bk"]).astype(np.float32), (rv + L["bv"]).astype(np.float32)
        rq, rk = rq.reshape(H, hd), rk.reshape(Hk, hd)
        if L["q_norm"] is not None:
            rq = np.stack([np_ref.rms_norm(r, L["q_norm"], ref.eps) for r in rq])
            rk = np.stack([np_ref.rms_norm(r, L["k_norm"], ref.eps) for r in rk])
        assert np.array_equal(ref._rope(rq, pos).astype(np.float16), q)
        assert np.array_equal(ref._rope(rk, pos).astype(np.float16), k)
        assert np.array_equal(rv.reshape(Hk, hd).astype(np.float16), v)


@pytest.mark.parametrize("preset", PRESETS)
def test_chunked_restatement_equals_plain_softmax(cases, preset):
    """The chunk / merge-batch structure in float64 is the plain softmax to rounding, far inside
    the bound (so a mutant's distance from the reference is the mutation's)."""
    _, C = cases[preset]
    for pattern, pos in (("flat", 65), ("peaked8", 513), ("peaked40", 1024), ("far_apart", 4096), ("census", 4096)):
        for h in (0, C.m.n_head - 1):
            q, K, V, out, bnd, _ = _head_case(C, pattern, pos, h, census=pattern == "census")
            assert _worst(A.chunked(q, K, V), out, bnd) < 1e-6
            assert np.isfinite(bnd).all() and (bnd > 0).all()


@pytest.mark.parametrize("preset", (5, 17))
def test_mutants_leave_the_bound(cases, preset):
    _, C = cases[preset]
    mod = C.m
    ratios = {}

    def mutant(name, pattern, pos, mut, arg=0, edit=None):
        worst = np.inf
        for h in (0, mod.n_head - 1):
            q, K, V, out, bnd, _ = _head_case(C, pattern, pos, h, edit, census=pattern == "census")
            worst = min(worst, _worst(A.chunked(q, K, V, mut, arg), out, bnd))
        ratios[f"{name} {pattern}@{pos}"] = worst

    for pos in (4096, 32767):
        last = A.CHUNK * (pos // A.CHUNK)
        mutant("drop 63", "census", pos, "drop", 63)
        mutant("drop 64", "census", pos, "drop", 64)
        mutant("drop first of last chunk", "census", pos, "drop", last)
        mutant("double 63", "census", pos, "double", 63)
        mutant("double last of a full chunk", "census", pos, "double", last - 1)
    mutant("P without lo", "flat_census", 63, "p_f16")
    for pos in (1023, 4096):
        mutant("no rescale", "far_apart", pos, "no_rescale")
    mutant("skip chunk 3", "census", 4096, "skip_chunk", 3)
    for pos in (513, 4096):
        for label, edit in C.edits("dominant", pos):
            mutant(f"skip chunk of {label}", "dominant", pos, "skip_chunk", edit[0][0] // A.CHUNK, edit)
    # the RoPE row of a neighbouring position, for q and the new k row alike
    for pattern, pos in (("flat", 65), ("flat", 4096), ("peaked8", 513)):
        for d in (-1, 1):
            worst = np.inf
            for h in (0, mod.n_head - 1):
                q, K, V, out, bnd, raw = _head_case(C, pattern, pos, h)
                q2, k2, _ = mod.prepare(0, raw, pos, rope_pos=pos + d)
                K[pos] = k2[h // mod.G]
                worst = min(worst, _worst(A.attend(q2[h], K, V)[0], out, bnd))
            ratios[f"rope {d:+d} {pattern}@{pos}"] = worst
    print(ratios)
    weak = {k: v for k, v in ratios.items() if not v > 1.0}
    assert not weak, weak
