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

Several tokens in one launch (tests/test_attention_multi_gpu.py; np_attn.multi and its mutants):
for every launch shape of that file (each prefill window, the full chunk, the admission list, the
batched step on 1, 3 and 16 slots) and every pattern it runs there, the unmutated reference
evaluated chunk-wise stays inside the bound, and every mutant that can occur in the shape leaves
the bound in at least one pattern (the GPU test runs all of them on the shape):

  a token also sees row pos + 1            every shape
  a token reads the injected row at pos    every shape (the injected rows are stale: np_attn.stale)
  a token's output lands in the next row   two tokens or more
  a token merges with a neighbour's        tokens with different chunk counts in one launch
  chunk count (no chunk 0)
  a token reads another sequence's cache   launches on batch slots (the handle's own cache is
                                           one sequence at offset 0: there is no other to read)
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


# ---------------------------------------------------------------- several tokens in one launch
def _multi_teeth(model, cases, mutants):
    """cases: [(label, caches, tokens)], one per pattern and sub-case of one launch shape. The
    unmutated reference, evaluated chunk-wise, stays inside the bound in every case; returns
    {mutant: {label: worst err / bound over the launch's outputs}}."""
    out = {mu: {} for mu in mutants}
    for label, caches, tokens in cases:
        att, bnd, _ = A.multi(model, caches, tokens)
        assert np.isfinite(bnd).all() and (bnd > 0).all(), label
        for t in {0, len(tokens) - 1}:  # the chunk / merge-batch restatement of the same launch
            sq, pos, raw = tokens[t]
            q = model.prepare(0, raw, pos)[0]
            K, V = caches[sq][0][:, :pos + 1].astype(np.float64), caches[sq][1][:, :pos + 1].astype(np.float64)
            for s2, p2, r2 in tokens:
                if s2 == sq and p2 <= pos:
                    _, K[:, p2], V[:, p2] = model.prepare(0, r2, p2)
            for h in (0, model.n_head - 1):
                kv = h // model.G
                assert _worst(A.chunked(q[h], K[kv], V[kv]), att[t, h], bnd[t, h]) < 1e-6, (label, t, h)
        for mu in mutants:
            out[mu][label] = _worst(A.multi(model, caches, tokens, mu)[0], att, bnd)
    return out


def _assert_teeth(ratios, where):
    """Every mutant leaves the bound in at least one pattern of the launch shape: the GPU test
    runs every pattern on it, so a kernel with that defect fails there."""
    print(where, {mu: {k: float(f"{v:.3g}") for k, v in r.items()} for mu, r in ratios.items()})
    weak = {mu: r for mu, r in ratios.items() if not max(r.values()) > 1.0}
    assert not weak, (where, weak)


def _window_mutants(p0, nt):
    mutants = ["see_next", "injected_row"]
    if nt > 1:
        mutants.append("neighbour_row")
    if p0 // A.CHUNK != (p0 + nt - 1) // A.CHUNK:  # tokens with different chunk counts
        mutants.append("skip_low_chunk")
    return mutants


@pytest.mark.parametrize("window", A.MULTI_WINDOWS, ids=lambda w: f"{w[0]}+{w[1]}")
@pytest.mark.parametrize("preset", (5, 17))
def test_multi_token_mutants_leave_the_bound(cases, preset, window):
    """The prefill windows of tests/test_attention_multi_gpu.py, every pattern: a token that also
    sees the row behind its position, that reads the cache's row at its position, whose output lands
    in the next row, or (windows across a chunk edge) that merges without its lowest chunk."""
    _, C = cases[preset]
    p0, nt = window
    runs = []
    for pattern in A.MULTI_PATTERNS:
        K16, V16 = C.state(pattern)
        tokens = A.window_tokens(C, pattern, p0, nt)
        for label, edit in A.window_edits(C, pattern, p0):
            K, V = K16[:, :p0 + nt + 1].copy(), V16[:, :p0 + nt + 1].copy()
            for t, kr, vr in edit:
                K[:, t], V[:, t] = kr, vr
            A.stale(V, p0, nt)
            runs.append((f"{pattern} {label}".strip(), {0: (K, V)}, tokens))
    _assert_teeth(_multi_teeth(C.m, runs, _window_mutants(p0, nt)), (preset, window))


@pytest.fixture(scope="module")
def slot_cases(cases):
    """Per preset, one Cases per slot (seed = slot + 1) at the short context of the multi-sequence
    launches."""
    return {p: [A.Cases(A.Model(cases[p][0]), seed=s + 1, n_ctx=A.MULTI_N_CTX) for s in range(max(A.STEP_SLOTS))]
            for p in (5, 17)}


@pytest.mark.parametrize("preset", (5, 17))
def test_multi_sequence_mutants_leave_the_bound(slot_cases, preset):
    """The full chunk, the flattened admission list and the batched step of the GPU test: beside the
    window mutants, a token that reads another sequence's cache."""
    S = slot_cases[preset]
    mod = S[0].m
    p0, nt = A.FULL_CHUNK
    runs = [(pattern, {0: A.slot_state(S[0], pattern, p0, nt)}, A.window_tokens(S[0], pattern, p0, nt))
            for pattern in A.FULL_PATTERNS]
    _assert_teeth(_multi_teeth(mod, runs, _window_mutants(p0, nt)), (preset, "full chunk"))
    runs = [(pattern,) + A.admission_case(S, pattern) for pattern in A.MULTI_PATTERNS]
    _assert_teeth(_multi_teeth(mod, runs, A.MULTI_MUTANTS), (preset, "admission"))
    for slots in A.STEP_SLOTS:
        runs = [(pattern,) + A.step_case(S, pattern, slots) for pattern in A.FULL_PATTERNS]
        # one token per sequence: the row behind it is the cache's; one slot has no neighbour
        mutants = ("see_next", "injected_row") if slots == 1 else A.MULTI_MUTANTS
        _assert_teeth(_multi_teeth(mod, runs, mutants), (preset, "step", slots))
