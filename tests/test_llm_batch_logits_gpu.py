"""GPU parity, bit level: the batched decode step's logits, K/V cache rows and short-conv rings
(mio_hip_llm_generate_batch / _generate_queue: launch_batch_step, csrc/hip/llm_prefill.hip) against
the single-stream decode of the same handle, at every engine LayerRun::plan can choose.

tests/test_llm_batch_gpu.py, test_llm_queue_gpu.py and test_sampler_gpu.py compare sampled token
ids, which a slightly wrong logits row rarely moves (T = 0.8 with Gumbel noise over 12 800 ids).
The design's claim is stronger (the same quantizers, per-superblock integer sums
in the same order, the same attention sweep), so here nothing has a tolerance: after a batched
call the slot states, the logits rows and every layer's cache rows are read back
(mio_hip_llm_batch_state / _batch_logits / _batch_kv_rows / _batch_conv_ring) and compared, as
uint32 / uint16 patterns, with a teacher-forced mio_hip_llm_eval loop over the same tokens.

Which row is which: a slot admitted with a prompt of L tokens starts at pos = step = L - 1 (the
queue's P: the prompt but for its last token is prefilled) and each of its n live steps decodes
the token at pos, writes cache row pos, samples and advances. After n steps the state is
pos = step = L - 1 + n, token = the id sampled last, cache rows [0, pos) are written and the logits
row is that of position pos - 1, the one the last id was sampled from. (The issue's text counted
pos one higher; the reference follows the reported pos.) The reference therefore evals
(prompt + sampled)[:pos] at positions 0 .. pos - 1 and keeps the last logits; the test asserts the
reported pos and step first, then derives everything from them.

Every cell asserts, from mio_debug_batch_plan (the launcher's own decisions, nothing launched),
that it reaches the engine it is there for; test_cells_cover_every_engine checks the union.

Shapes the table's text left open:
- the Q8_0 model at n_embd 576 is preset 0's file rules with preset 2's width, heads 9 / 3 and
  n_ff 1536 (preset 2 itself has the 61 952-id vocabulary; its head shape is the one
  test_llm_batch_gpu.py's (2, 3) case already runs);
- n_embd 2304 keeps head_dim 64 and 2 query heads per kv head with 36 / 18 heads, so that
  n_head * head_dim stays n_embd;
- its n_ff is 2304 (the table leaves it open).
"""
import numpy as np
import pytest

import miotts_amd as m
import pyoracle

pytestmark = pytest.mark.gpu

ALLOW = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800)
N_NEW = 12
N_CTX = 256

# name -> (preset, recipe, n_embd, n_layer, n_head, n_head_kv, n_ff); 0 keeps the preset's
MODELS = {
    "q8": (0, 8, 256, 2, 0, 0, 512),
    "q8_ff2304": (0, 8, 256, 2, 0, 0, 2304),
    "q8_ff6400": (0, 8, 256, 2, 0, 0, 6400),
    "q8_e576": (0, 8, 576, 2, 9, 3, 1536),
    "k15": (1, 15, 256, 2, 0, 0, 2304),
    "k17": (1, 17, 256, 2, 0, 0, 2304),
    "k18": (1, 18, 256, 2, 0, 0, 2304),
    "k12": (1, 12, 256, 2, 0, 0, 2304),
    "k15_ff6400": (1, 15, 256, 2, 0, 0, 6400),
    "k15_e2304": (1, 15, 2304, 2, 36, 18, 2304),
    "bf16": (11, None, 0, 0, 0, 0, 0),
    "lfm2_q8": (7, None, 0, 0, 0, 0, 0),
    "lfm2_k15": (8, None, 0, 0, 0, 0, 0),
}
Q8_MODELS = {"q8", "q8_ff2304", "q8_ff6400", "q8_e576", "lfm2_q8"}

CELLS = ([("q8", B) for B in (1, 3, 8, 9, 16)] + [("q8_ff2304", B) for B in (8, 9, 16)] +
         [("q8_ff6400", B) for B in (8, 9, 16)] + [("q8_e576", B) for B in (3, 9)] +
         [(k, B) for k in ("k15", "k17", "k18", "k12") for B in (3, 8, 9, 16)] +
         [("k15_ff6400", B) for B in (8, 16)] + [("k15_e2304", B) for B in (3, 9)] +
         [("bf16", B) for B in (3, 9)] + [(k, B) for k in ("lfm2_q8", "lfm2_k15") for B in (3, 9)])

MATRIX_CORES = ("mmq", "mmq_q")
QKV, O, GATE_UP, DOWN = 0, 1, 2, 3


class _Models:
    """The shaped model files, and one loaded handle per (model, n_ctx): the batch state
    re-allocates on a new B, the weights stay."""

    def __init__(self, device, tmp):
        self.device, self.tmp, self.paths, self.handles = device, tmp, {}, {}

    def path(self, name):
        if name not in self.paths:
            preset, recipe, n_embd, n_layer, n_head, n_kv, n_ff = MODELS[name]
            p = str(self.tmp / f"{name}.gguf")
            if recipe is None:
                m.synth_llm(p, preset, 1)
            else:
                m.synth_llm_shape(p, preset, recipe, 1, n_embd, n_layer, n_head, n_kv, n_ff)
            self.paths[name] = p
        return self.paths[name]

    def llm(self, name, n_ctx=N_CTX):
        if (name, n_ctx) not in self.handles:
            g = m.Llm(self.device, self.path(name), n_ctx)
            g.conv_layers = [il for il in range(g.n_layer) if _is_conv(g, il)]
            g.attn_layers = [il for il in range(g.n_layer) if il not in g.conv_layers]
            self.handles[(name, n_ctx)] = g
        return self.handles[(name, n_ctx)]

    def close(self):
        for g in self.handles.values():
            g.close()


def _is_conv(g, il):
    try:
        g.conv_ring(il)
        return True
    except m.HipError:
        return False


@pytest.fixture(scope="module")
def models(device, tmp_path_factory):
    ms = _Models(device, tmp_path_factory.mktemp("llm_batch_logits"))
    yield ms
    ms.close()


def _prompt(b, single_token):
    """Slot b's prompt, the same whatever B: 3 to 40 byte tokens, or one token."""
    rng = np.random.default_rng(4000 + b)
    n = 1 if single_token else int(rng.integers(3, 41))
    return [int(t) for t in rng.integers(0, 256, n)]


def _prompts(B):
    # ragged lengths and a 1-token prompt (nothing to prefill for that slot) wherever B > 1
    return [_prompt(b, b == 1) for b in range(B)]


def _seeds(B):
    return [1000 + 17 * b for b in range(B)]


def _named(site):
    return (m.PLAN_ENGINES[site[0]], m.PLAN_SHAPES[site[1]], site[2])


def _plan(g, B):
    sites, lm = g.batch_plan(B)
    return [[_named(s) for s in row] for row in sites], _named(lm)


# ---------------------------------------------------------------- the reference, computed once
_REF = {}


def _single_stream(g, key, toks):
    """Teacher-forced single-stream decode of toks at positions 0 .. len - 1 on handle g: the last
    logits, rows [0, len) of every attention layer and every short-conv ring. Kept per token list
    (slot b's prompt and seed do not depend on B, so one run serves every B of a model)."""
    key = (key, tuple(toks))
    if key not in _REF:
        for i, t in enumerate(toks):
            lg = g.eval(int(t), i)
        _REF[key] = (lg, {il: g.kv_rows(il, len(toks)) for il in g.attn_layers},
                     {il: g.conv_ring(il) for il in g.conv_layers})
    return _REF[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _first_kv_diff(b, il, got, ref):
    """(slot, layer, position, 'k' / 'v') of the first differing cache row, or None."""
    for which, gr, rr in (("k", got[0], ref[0]), ("v", got[1], ref[1])):
        bad = (_bits(gr) != _bits(rr)).any(axis=(0, 2))
        if bad.any():
            return (b, il, int(np.argmax(bad)), which)
    return None


def _compare_slot(g, b, n_rows, ref, logits_row, report):
    """Slot b of the batch state against the reference (logits, kv, rings): cache rows [0, n_rows)
    of every attention layer, every ring (None: not compared), the logits row. Appends to report."""
    ref_lg, ref_kv, ref_ring = ref
    for il in g.attn_layers:
        k, v = g.batch_kv_rows(b, il, n_rows)
        d = _first_kv_diff(b, il, (k, v), (ref_kv[il][0][:, :n_rows], ref_kv[il][1][:, :n_rows]))
        if d:
            report.append(f"first differing cache row (slot, layer, position, k/v): {d}")
            break
    for il in (g.conv_layers if ref_ring is not None else []):
        if not np.array_equal(_bits(g.batch_conv_ring(b, il)), _bits(ref_ring[il])):
            report.append(f"short-conv ring differs (slot, layer): {(b, il)}")
            break
    if not np.array_equal(_bits(logits_row), _bits(ref_lg)):
        d = np.abs(logits_row.astype(np.float64) - ref_lg)
        report.append(f"logits differ (slot {b}): {int((_bits(logits_row) != _bits(ref_lg)).sum())} of "
                      f"{ref_lg.size}, largest |diff| {d.max():.3g} at id {int(d.argmax())} "
                      f"(max |logit| {np.abs(ref_lg).max():.3g})")


# ---------------------------------------------------------------- a cell, run once
_CELL = {}


def _cell(models, name, B):
    """generate_batch of B ragged prompts x N_NEW tokens on the model, and what it left behind."""
    if (name, B) not in _CELL:
        g = models.llm(name)
        prompts, seeds = _prompts(B), _seeds(B)
        got = g.generate_batch(prompts, N_NEW, 0.8, seeds, allow=ALLOW)
        _CELL[(name, B)] = (prompts, got, g.batch_state(), g.batch_logits())
    return _CELL[(name, B)]


def _check_plan(name, B, sites, lm):
    """The engines the cell is there for (the table of the issue), from the plan report."""
    engines = [s[0] for row in sites for s in row]
    if name == "q8":
        if B <= 8:
            for row in sites:
                assert row[QKV] == ("mmq_q", "qkv", 1) and row[GATE_UP] == ("mmq_q", "gate_up", 1), row
        else:
            assert all(e in MATRIX_CORES for e in engines), sites
    elif name == "q8_ff2304":
        for row in sites:
            if B <= 8:
                assert row[DOWN][0] in ("dot4", "dot4_down_q"), row
            else:
                assert row[DOWN] == ("mmq_q", "down_q8", 3), row
    elif name == "q8_ff6400":
        for row in sites:
            assert row[GATE_UP] == ("mmq_q", "gate_up_walk", 1), row
            if B > 8:
                assert row[DOWN] == ("mmq_q", "down_q8", 6), row
    elif name == "q8_e576":
        for row in sites:
            if B <= 8:
                assert row[QKV][0] == "dot4_xpre" and row[GATE_UP][0] == "dot4_xpre", row
            else:
                # 576 is no multiple of 256: no fused shape, the generic tiles of launch_mmq
                assert row[QKV] == ("mmq_q", "none", 1) and row[GATE_UP] == ("mmq_q", "none", 1), row
                assert all(s[0] in MATRIX_CORES for s in row), row
    elif name in ("k15", "k17", "k18", "k12"):
        assert all(e in MATRIX_CORES for e in engines), sites
        for row in sites:
            assert row[QKV] == ("mmq_q", "qkv", 1) and row[DOWN] == ("mmq_q", "down_kq", 3), row
            assert row[GATE_UP] == ("mmq_q", "gate_up", 1), row
    elif name == "k15_ff6400":
        for row in sites:
            assert row[GATE_UP] == ("mmq_q", "gate_up_walk", 1) and row[DOWN] == ("mmq_q", "none", 6), row
    elif name == "k15_e2304":
        for row in sites:
            assert row[QKV] == ("mmq_q", "none", 3) and row[GATE_UP] == ("mmq_q", "none", 3), row
    elif name == "bf16":
        assert all(e == "dot4" for e in engines) and lm[0] == "dot4", (sites, lm)
    else:  # lfm2: conv-in and conv-out on the matrix cores over act records
        assert name in ("lfm2_q8", "lfm2_k15")


def _tags(name, sites):
    """What a cell contributes to the coverage union."""
    t = set()
    for row in sites:
        for j, (e, shape, np_) in enumerate(row):
            t.add(e if e != "mmq_q" else ("mmq_q fused" if shape != "none" else "mmq_q not fused"))
            if shape == "down_q8":
                t.add(f"q8 down fused np {np_}")
            if shape == "gate_up_walk":
                t.add("gate|up walk " + ("q8" if name in Q8_MODELS else "kq"))
    return t


@pytest.mark.parametrize("name,B", CELLS)
def test_batch_step_bits_equal_single_stream(models, name, B):
    g = models.llm(name)
    sites, lm = _plan(g, B)
    print(name, B, sites, lm)
    _check_plan(name, B, sites, lm)
    if name.startswith("lfm2"):
        assert g.conv_layers and g.attn_layers
        for il in g.conv_layers:
            assert sites[il][0][0] == "mmq" and sites[il][1][0] == "mmq", sites[il]
    prompts, got, st, logits = _cell(models, name, B)
    report = []
    for b in range(B):
        L = len(prompts[b])
        assert len(got[b]) == N_NEW, (b, got[b])
        # the reported state first; everything below is derived from it
        assert (st["pos"][b], st["step"][b], st["token"][b], st["done"][b]) == \
            (L - 1 + N_NEW, L - 1 + N_NEW, got[b][-1], 0), (b, {k: int(v[b]) for k, v in st.items()})
        pos = int(st["pos"][b])
        toks = (prompts[b] + [int(t) for t in got[b]])[:pos]
        assert toks[-1] == got[b][-2] and len(toks) == L + N_NEW - 1
        _compare_slot(g, b, pos, _single_stream(g, name, toks), logits[b], report)
    assert not report, "\n".join(report)


@pytest.mark.parametrize("name,B", [("q8", 1), ("k15", 3)])
def test_batch_logits_anchor_to_oracle(models, name, B):
    """The first Q8_0 and the first Q4_K_M cell: slot 0's batched logits against the C oracle
    teacher-forced over the same tokens, max |diff| <= 5e-2 max |logits|
    (test_batched_prefill_matches_sequential's bound), so the file does not rest on the GPU alone."""
    prompts, got, st, logits = _cell(models, name, B)
    toks = (prompts[0] + [int(t) for t in got[0]])[:int(st["pos"][0])]
    o = pyoracle.Llm(models.path(name), N_CTX)
    for i, t in enumerate(toks):
        ref = o.eval(int(t), i)
    err, scale = float(np.abs(logits[0] - ref).max()), float(np.abs(ref).max())
    print(f"{name}: max |diff| {err:.3g}, max |logit| {scale:.3g}")
    assert err <= 5e-2 * scale, (err, scale)


def test_frozen_slots_repeat_their_step(models):
    """Budgets made ragged by the context: n_ctx 64, prompts of 8, 60, 60 and 30 tokens,
    max_tokens 24: slots 1 and 2 have a budget of 64 - 60 + 1 = 5 tokens and are stepped 19 more
    times, frozen on the last cache row (pos 63). A frozen step must be idempotent: its logits row
    equals eval(last sampled token, reported pos) on caches that equal the teacher-forced ones
    below that position, and it stays out of its neighbours' caches (slots 0 and 3 are compared as
    in the cells)."""
    g = models.llm("q8", 64)
    rng = np.random.default_rng(64)
    prompts = [[int(t) for t in rng.integers(0, 256, n)] for n in (8, 60, 60, 30)]
    got = g.generate_batch(prompts, 24, 0.8, _seeds(4), allow=ALLOW)
    assert [len(t) for t in got] == [24, 5, 5, 24]
    st, logits = g.batch_state(), g.batch_logits()
    report = []
    for b in range(4):
        L, n = len(prompts[b]), len(got[b])
        pos = int(st["pos"][b])
        assert pos == min(L - 1 + n, 63) and st["token"][b] == got[b][-1] and st["done"][b] == 0, (b, st)
        assert st["step"][b] == L - 1 + n
        toks = (prompts[b] + [int(t) for t in got[b]])[:pos]
        ref_lg, ref_kv, _ = _single_stream(g, "q8@64", toks)
        if n < 24:  # frozen: the repeated step decodes the last sampled token at pos
            ref_lg = g.eval(int(got[b][-1]), pos)
        _compare_slot(g, b, pos, (ref_lg, ref_kv, None), logits[b], report)
    assert not report, "\n".join(report)


def test_refilled_slots_bits_equal_single_stream(models):
    """generate_queue, 9 utterances on 3 slots, budgets ragged by the context as in
    test_queue_ragged_by_context_budget_and_step_count (n_ctx 128: prompts of 8 / 120 / 120 tokens,
    budgets 120 / 9 / 9): after the call the last utterance of each slot has its single-stream
    logits and cache rows, bit for bit: the previous tenants' rows above its length are read by
    nothing. A slot whose last utterance ended before the call did has run frozen steps since: its
    logits row is then that of (last token, pos), as in test_frozen_slots_repeat_their_step."""
    g = models.llm("k15", 128)
    rng = np.random.default_rng(9)
    plens, budgets = [8, 120, 120] * 3, [120, 9, 9] * 3
    prompts = [[int(t) for t in rng.integers(0, 256, n)] for n in plens]
    got, stats = g.generate_queue(prompts, 120, 0.8, [40 + u for u in range(9)], slots=3, allow=ALLOW)
    print(stats)
    assert [len(t) for t in got] == budgets
    st, logits = g.batch_state(), g.batch_logits()
    report = []
    for b in range(3):
        u = max(v for v in range(9) if stats["slot_of"][v] == b)
        L, n = plens[u], budgets[u]
        frozen = stats["steps"] - stats["start_step"][u] - n
        assert frozen >= 0
        pos = int(st["pos"][b])
        assert pos == min(L - 1 + n, 127) and st["step"][b] == L - 1 + n and st["token"][b] == got[u][-1], (b, u, st)
        toks = (prompts[u] + [int(t) for t in got[u]])[:pos]
        ref_lg, ref_kv, _ = _single_stream(g, "k15@128", toks)
        if frozen:
            ref_lg = g.eval(int(got[u][-1]), pos)
        elif pos < L - 1 + n:  # ended at the full context with no step after: the row of position pos
            ref_lg = g.eval(int(got[u][-2]), pos)
        _compare_slot(g, b, pos, (ref_lg, ref_kv, None), logits[b], report)
    assert not report, "\n".join(report)


def test_cells_cover_every_engine(models):
    """The union over the cells, from the plan report: every engine of LayerRun::plan, kMmqQ both
    with a fused kernel and on its fall-back, the fused Q8_0 down of 3 and of 6 passes, and the
    gate|up tile walk in Q8_0 and in a K-quant."""
    seen = set()
    for name, B in CELLS:
        seen |= _tags(name, _plan(models.llm(name), B)[0])
    need = {"dot4", "dot4_xpre", "dot4_down_q", "mmq", "mmq_q fused", "mmq_q not fused", "q8 down fused np 3",
            "q8 down fused np 6", "gate|up walk q8", "gate|up walk kq"}
    assert need <= seen, sorted(need - seen)
