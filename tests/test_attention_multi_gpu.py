"""GPU parity: the multi-token engine's attention launches (k_pf_rope + k_pf_attention of the chunked
prefill and the queue's admissions, k_bt_attention of the batched decode step;
csrc/hip/llm_prefill.hip) alone, on injected K/V states and raw q|k|v rows, against the float64
reference np_attn.multi under np_attn.bound (the error model derived in test_attention_gpu.py; no
other tolerance: everything else here is equality of bit patterns).

One call of mio_hip_llm_debug_attention_multi per launch: LayerRun::attention of layer 0 for nt
tokens, with the per-token pos / seq lists, the seq_kv cache offset, row pos read back from the
cache (mode 0) or staged from LDS (mode 1), the causal mask among rows that were all written before
any token attends, one ticket per (token, kv head) with a chunk count of the token's own, the early
exit of chunks past a token's position, the frozen-slot skip and the merger's activation records.
Head shapes: presets 5, 9, 17, 18 (test_attention_gpu.py's). The raw rows are nudged, so the K/V
rows the launches append equal the reference's bit for bit.

  a  prefill windows on the 32768-row cache (np_attn.MULTI_WINDOWS x MULTI_PATTERNS): att against
     float64; cache rows [0, window end + 64) of layer 0 bit-equal to the injected state with the
     window's rows replaced by the reference's; the same rows of layer 1 unchanged; att rows
     bit-equal to the single-stream launch (mio_hip_llm_debug_attention, which = 1) run token by
     token on the restored state ("pb.att holds the decode's outputs bit for bit");
  b  a full chunk of 128 tokens ending at the last row of a 2048-row cache;
  c  poison: the rows behind the window in its chunk as f16 NaN / +Inf / -Inf give the zero-filled
     call's bits; so do poisoned rows of a slot the launch does not address;
  d  a flattened admission list: three sequences interleaved in one mode-0 launch on three slots;
  e  the batched step on 1, 3 and 16 slots at ragged positions: float64, bit-equal to a mode-0
     launch of the same tokens and to the single-stream launch on the slot's state; two frozen
     slots leave sentinel rows, untouched caches and zero tickets; every position below 64 under the
     step's full chunk count;
  f  every ticket is 0 after every launch here, and a second launch on the tickets the first left
     gives its bits;
  g  the merger's records (att_q 0 on every shape, 1 where G * hd = 256): att bits as without
     them, qs / d / bs equal to np_act_quant of the att row and to mio_hip_debug_act_quant of it
     ("the records are k_bt_quant's bits"), with an all-zero kv head and a +- tied maximum;
  h  refusals.

Measured on the MI355X, worst err / bound per pattern over the four shapes:

  mode 0 windows       census 0.0054   flat_census 0.0080   peaked40 0.12   dominant 0.0031
                       far_apart 0.0031   vsubnormal 0.0046
  mode 0 full chunk    census 0.0033   peaked40 0.0038
  mode 0 admission     census 0.0065   flat_census 0.0057   peaked40 0.025   dominant 0.0022
                       far_apart 0.0045   vsubnormal 0.0056
  mode 1 batched step  census 0.0062   peaked40 0.14 (16 slots; 0.034 on 3, 0.025 on 1)

Every bit comparison held on the first run: no defect found in the launches. The rows a launch
overwrites are injected stale (np_attn.stale), since the census row of a position is the very row
its token appends; tests/test_attention_ref.py shows the mutants these cases reject.
"""
import numpy as np
import pytest

import miotts_amd as m
import np_act_quant as aq
import np_attn as A

pytestmark = pytest.mark.gpu

PRESETS = (5, 9, 17, 18)
SENTINEL = 0x7FC5A5A5  # MIO_DEBUG_SENTINEL_F32
POISON = (("nan", 0x7E00), ("inf", 0x7C00), ("-inf", 0xFC00))

_long, _short, _loaded = {}, {}, {}


def _u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _other_layer(g, n_ctx):
    """Layer 1 (where the model has one) holds rows of its own, so that a write there shows."""
    if g.n_layer > 1:
        rows = np.random.default_rng(9).integers(0, 0x7C00, (g.n_kv, n_ctx, g.head_dim)).astype(np.uint16)
        g.set_kv_rows(1, 0, rows.view(np.float16), rows.view(np.float16))


@pytest.fixture(scope="module")
def long_models(device, synth_llm_path):
    """preset -> (Llm at n_ctx 32768, Cases): the prefill windows on the handle's own cache."""
    def get(preset):
        if preset not in _long:
            path = synth_llm_path(preset)
            g = m.Llm(device, path, A.N_CTX)
            _other_layer(g, A.N_CTX)
            _long[preset] = (g, A.Cases(A.Model(path)))
        return _long[preset]

    yield get
    for g, _ in _long.values():
        g.close()
    _long.clear()
    _loaded.clear()


@pytest.fixture(scope="module")
def short_models(device, synth_llm_path):
    """preset -> (Llm at n_ctx 2048 with 16 batch slots, [Cases of slot s, seed s + 1])."""
    def get(preset):
        if preset not in _short:
            path = synth_llm_path(preset)
            g = m.Llm(device, path, A.MULTI_N_CTX)
            _other_layer(g, A.MULTI_N_CTX)
            mod = A.Model(path)
            S = [A.Cases(mod, seed=s + 1, n_ctx=A.MULTI_N_CTX) for s in range(max(A.STEP_SLOTS))]
            # the batch state of 16 slots (the first call with slots > 0 allocates it, zeroed)
            g.debug_attention_multi(0, 1, max(A.STEP_SLOTS), [0], [0], S[0].raw(0))
            _short[preset] = (g, S)
        return _short[preset]

    yield get
    for g, _ in _short.values():
        g.close()
    _short.clear()


# ---------------------------------------------------------------- device state and launches
def _put(g, slot, K, V, lo, hi):
    """Rows [lo, hi) of the host state into layer 0 of the handle's cache (slot None) or a slot's."""
    if hi <= lo:
        return
    if slot is None:
        g.set_kv_rows(0, lo, K[:, lo:hi], V[:, lo:hi])
    else:
        g.batch_set_kv_rows(slot, 0, lo, K[:, lo:hi], V[:, lo:hi])


def _get(g, slot, n, il=0):
    return g.kv_rows(il, n) if slot is None else g.batch_kv_rows(slot, il, n)


def _launch(g, mode, slots, tokens, **kw):
    """One launch of the tokens [(seq, pos, raw)]; every ticket is 0 after it (f)."""
    att, rec, tickets = g.debug_attention_multi(0, mode, slots, [p for _, p, _ in tokens], [s for s, _, _ in tokens],
                                                np.stack([r for _, _, r in tokens]), **kw)
    assert not tickets.any(), tickets
    return att, rec


def _restore(g, slots, caches, tokens):
    """The tokens' cache rows back to the injected state."""
    for s, p, _ in tokens:
        _put(g, s if slots else None, caches[s][0], caches[s][1], p, p + 1)


def _check_rows(g, slots, caches, tokens, rows, other=None):
    """Every row of the host states bit-equal on the device, the tokens' rows replaced by the
    reference's; other: (layer 1 rows before the launch) unchanged."""
    for s, (K, V) in caches.items():
        wk, wv = K.copy(), V.copy()
        for (s2, p, _), (k, v) in zip(tokens, rows):
            if s2 == s:
                wk[:, p], wv[:, p] = k, v
        kg, vg = _get(g, s if slots else None, K.shape[1])
        bad = np.flatnonzero((_u16(kg) != _u16(wk)).any(axis=(0, 2)) | (_u16(vg) != _u16(wv)).any(axis=(0, 2)))
        assert bad.size == 0, (s, bad[:8])
    if other is not None:
        k1, v1 = _get(g, None, other[0].shape[1], 1)
        assert np.array_equal(_u16(k1), _u16(other[0])) and np.array_equal(_u16(v1), _u16(other[1]))


def _check(g, mod, mode, slots, caches, tokens, label, **kw):
    """The launch against float64 and its cache rows; returns (att, worst err / bound)."""
    ref, bnd, rows = A.multi(mod, caches, tokens)
    n1 = max(K.shape[1] for K, _ in caches.values())
    other = _get(g, None, n1, 1) if slots == 0 and g.n_layer > 1 else None
    att, _ = _launch(g, mode, slots, tokens, **kw)
    _check_rows(g, slots, caches, tokens, rows, other)
    assert np.isfinite(att).all(), label
    ratio = np.abs(att - ref) / bnd
    assert ratio.max() <= 1.0, (label, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
    return att, float(ratio.max())


def _single_stream(g, caches, tokens, att, label):
    """att rows bit-equal to the decode's attention launch, token by token in ascending position on
    the handle's own cache (which holds the tokens' sequence up to each position)."""
    for t in sorted(range(len(tokens)), key=lambda t: tokens[t][1]):
        _, pos, raw = tokens[t]
        one = g.debug_attention(0, pos, 1, raw)
        assert one.tobytes() == att[t].tobytes(), (label, pos, int((_u32(one) != _u32(att[t])).sum()))


def _load_long(g, C, preset, pattern):
    """The whole state of a pattern in layer 0 of the 32768-row cache (kept between cases: every
    case puts the rows it changed back)."""
    if _loaded.get(preset, (None,))[0] != pattern:
        K16, V16 = C.state(pattern)
        g.set_kv_rows(0, 0, K16, V16)
        _loaded[preset] = (pattern, K16, V16)
    return _loaded[preset][1:]


def _window(g, C, preset, pattern, p0, nt, K16, V16, what):
    """Checks a (and b) of one window on the handle's own cache, which holds K16 / V16."""
    hi = min(p0 + nt + A.CHUNK, K16.shape[1])
    tokens = A.window_tokens(C, pattern, p0, nt)
    worst = 0.0
    for label, edit in A.window_edits(C, pattern, p0):
        K, V = K16[:, :hi].copy(), V16[:, :hi].copy()
        for t, kr, vr in edit:
            K[:, t], V[:, t] = kr, vr
            _put(g, None, K, V, t, t + 1)
        A.stale(V, p0, nt)  # the window's own rows hold something else than the launch writes
        _put(g, None, K, V, p0, p0 + nt)
        caches = {0: (K, V)}
        att, w = _check(g, C.m, 0, 0, caches, tokens, (pattern, label, p0))
        worst = max(worst, w)
        _restore(g, 0, caches, tokens)
        _single_stream(g, caches, tokens, att, (pattern, label, p0))
        for t in [t for t, _, _ in edit] + list(range(p0, p0 + nt)):
            _put(g, None, K16, V16, t, t + 1)
    print(f"multi attention {what} preset {preset} {pattern} [{p0}..{p0 + nt - 1}]: worst err/bound {worst:.3g}")


# ---------------------------------------------------------------- a, b: prefill windows
@pytest.mark.parametrize("window", A.MULTI_WINDOWS, ids=lambda w: f"{w[0]}+{w[1]}")
@pytest.mark.parametrize("pattern", A.MULTI_PATTERNS)
@pytest.mark.parametrize("preset", PRESETS)
def test_prefill_window(long_models, preset, pattern, window):
    g, C = long_models(preset)
    K16, V16 = _load_long(g, C, preset, pattern)
    _window(g, C, preset, pattern, window[0], window[1], K16, V16, "window")


@pytest.mark.parametrize("pattern", A.FULL_PATTERNS)
@pytest.mark.parametrize("preset", PRESETS)
def test_full_chunk(short_models, preset, pattern):
    g, S = short_models(preset)
    K16, V16 = S[0].state(pattern)
    g.set_kv_rows(0, 0, K16, V16)
    _window(g, S[0], preset, pattern, A.FULL_CHUNK[0], A.FULL_CHUNK[1], K16, V16, "full chunk")


# ---------------------------------------------------------------- c: poison
@pytest.mark.parametrize("window", ((60, 8), (32760, 8)), ids=lambda w: f"{w[0]}+{w[1]}")
@pytest.mark.parametrize("preset", PRESETS)
def test_poison_behind_the_window(long_models, preset, window):
    g, C = long_models(preset)
    pattern = "flat_census"
    K16, V16 = _load_long(g, C, preset, pattern)
    p0, nt = window
    end = min(A.CHUNK * ((p0 + nt - 1) // A.CHUNK + 1), A.N_CTX)  # the end of the last token's chunk
    tokens = A.window_tokens(C, pattern, p0, nt)
    shape = (C.m.n_kv, end - p0, C.m.hd)
    fill = lambda bits: (np.full(shape, bits, np.uint16).view(np.float16),) * 2

    def run(bits, slots, slot):
        """The rows behind the window (slot None / 0), or the window's rows and those behind it
        (another slot), filled; the launch on the window."""
        k, v = fill(bits)
        lo = p0 + nt if slot in (None, 0) else p0
        if end > lo:
            (g.set_kv_rows(0, lo, k[:, lo - p0:], v[:, lo - p0:]) if slot is None else
             g.batch_set_kv_rows(slot, 0, lo, k[:, lo - p0:], v[:, lo - p0:]))
        att, _ = _launch(g, 0, slots, tokens)
        if slot not in (None, 0):  # the other slot keeps its rows
            kg, vg = g.batch_kv_rows(slot, 0, end)
            assert (_u16(kg[:, lo:]) == bits).all() and (_u16(vg[:, lo:]) == bits).all()
        return att

    zero = run(0, 0, None)
    for name, bits in POISON:
        assert run(bits, 0, None).tobytes() == zero.tobytes(), (name, "own cache")
    _put(g, None, K16, V16, p0, end)
    # slot 0 of two slots holds the state's rows up to the chunk's end; slot 1 is not addressed
    g.debug_attention_multi(0, 0, 2, [0], [0], C.raw(0))  # the batch state, where the handle has none
    g.batch_set_kv_rows(0, 0, 0, K16[:, :end], V16[:, :end])
    run(0, 2, 0)
    zero2 = run(0, 2, 1)
    assert zero2.tobytes() == zero.tobytes()  # the slot's cache gives the handle's own cache's bits
    for name, bits in POISON:
        g.batch_set_kv_rows(0, 0, p0, K16[:, p0:p0 + nt], V16[:, p0:p0 + nt])
        assert run(bits, 2, 1).tobytes() == zero.tobytes(), (name, "other slot")
        assert run(bits, 2, 0).tobytes() == zero.tobytes(), (name, "slot 0")


# ---------------------------------------------------------------- d: flattened admission lists
def _inject(g, caches):
    for s, (K, V) in caches.items():
        g.batch_set_kv_rows(s, 0, 0, K, V)


@pytest.mark.parametrize("pattern", A.MULTI_PATTERNS)
@pytest.mark.parametrize("preset", PRESETS)
def test_admission_list(short_models, preset, pattern):
    g, S = short_models(preset)
    caches, tokens = A.admission_case(S, pattern)
    _inject(g, caches)
    _, w = _check(g, S[0].m, 0, 3, caches, tokens, pattern)
    print(f"multi attention admission preset {preset} {pattern}: worst err/bound {w:.3g}")


# ---------------------------------------------------------------- e: the batched step
@pytest.mark.parametrize("slots", A.STEP_SLOTS)
@pytest.mark.parametrize("pattern", A.FULL_PATTERNS)
@pytest.mark.parametrize("preset", PRESETS)
def test_batched_step(short_models, preset, pattern, slots):
    g, S = short_models(preset)
    mod = S[0].m
    caches, tokens = A.step_case(S, pattern, slots)
    _inject(g, caches)
    att, w = _check(g, mod, 1, slots, caches, tokens, (pattern, slots))
    print(f"multi attention step preset {preset} {pattern} B={slots}: worst err/bound {w:.3g}")
    _restore(g, slots, caches, tokens)
    assert _launch(g, 0, slots, tokens)[0].tobytes() == att.tobytes()  # the prefill pair on the same tokens
    for t, (s, pos, raw) in enumerate(tokens):  # the single stream on the slot's state
        g.set_kv_rows(0, 0, caches[s][0][:, :pos + 1], caches[s][1][:, :pos + 1])
        assert g.debug_attention(0, pos, 1, raw).tobytes() == att[t].tobytes(), (s, pos)
    if slots < 3:
        return
    frozen = np.zeros(slots, np.int32)
    frozen[[1, slots - 2]] = 1
    _restore(g, slots, caches, tokens)
    att_f, _ = _launch(g, 1, slots, tokens, frozen=frozen)
    live = frozen == 0
    assert (_u32(att_f[~live]) == SENTINEL).all()
    assert att_f[live].tobytes() == att[live].tobytes()
    ref_rows = A.multi(mod, caches, tokens)[2]
    # a frozen slot's cache is the injected state, row pos included; a live one has its new row
    _check_rows(g, slots, {s: caches[s] for s in range(slots) if frozen[s]}, [], [])
    _check_rows(g, slots, {s: caches[s] for s in range(slots) if live[s]}, tokens, ref_rows)


@pytest.mark.parametrize("preset", PRESETS)
def test_batched_step_sweeps_every_chunk_of_short_sequences(short_models, preset):
    """Every position below 64 while the grid has the step's ceil(n_ctx / 64) chunks: all but the
    first exit at once, and each (token, kv head) ticket counts one arrival."""
    g, S = short_models(preset)
    caches, tokens = A.step_case(S, "census", 3, [0, 1, 63])
    _inject(g, caches)
    att, _ = _check(g, S[0].m, 1, 3, caches, tokens, "short", n_chunks=A.MULTI_N_CTX // A.CHUNK)
    _restore(g, 3, caches, tokens)
    assert _launch(g, 1, 3, tokens)[0].tobytes() == att.tobytes()  # n_chunks 0: the same count
    _restore(g, 3, caches, tokens)
    assert _launch(g, 0, 3, tokens, n_chunks=1)[0].tobytes() == att.tobytes()


# ---------------------------------------------------------------- f: tickets
@pytest.mark.parametrize("preset", PRESETS)
def test_second_launch_on_the_tickets_the_first_left(long_models, short_models, preset):
    g, C = long_models(preset)
    _load_long(g, C, preset, "peaked40")
    K16, V16 = _loaded[preset][1:]
    for p0, nt in ((60, 8), (505, 16)):
        tokens = A.window_tokens(C, "peaked40", p0, nt)
        first, _ = _launch(g, 0, 0, tokens, reset=True)
        again, _ = _launch(g, 0, 0, tokens, reset=False)
        assert again.tobytes() == first.tobytes(), (p0, nt)
        _put(g, None, K16, V16, p0, p0 + nt)
    g, S = short_models(preset)
    caches, tokens = A.step_case(S, "peaked40", 16)
    _inject(g, caches)
    first, _ = _launch(g, 1, 16, tokens, reset=True)
    again, _ = _launch(g, 1, 16, tokens, reset=False)
    assert again.tobytes() == first.tobytes()


# ---------------------------------------------------------------- g: the merger's records
def _check_records(device, att, rec, att_q, label):
    """qs[0:K], d and (Q8_K) bs of every token's record: np_act_quant of the att row the call
    returned, and mio_hip_debug_act_quant of it (no norm)."""
    for t in range(att.shape[0]):
        row = att[t].reshape(-1)
        K = row.size
        if att_q == 0:
            qs, d = aq.q8_0(row)
            gq, gd, _ = m.debug_act_quant(device, 8, row, None, 1e-6, False)
            nd = K // 32
        else:
            qs, d, bs = aq.q8_k(row)
            gq, gd, gb = m.debug_act_quant(device, 12, row, None, 1e-6, False)
            nd = K // 256
            assert np.array_equal(rec["bs"][t, :K // 16], bs), (label, t, "bsums")
            assert np.array_equal(rec["bs"][t, :K // 16], gb[:K // 16]), (label, t, "bsums / act_quant")
        assert np.array_equal(rec["qs"][t, :K], qs), (label, t, "codes", int((rec["qs"][t, :K] != qs).sum()))
        assert np.array_equal(_u32(rec["d"][t, :nd]), _u32(d)), (label, t, "d")
        assert np.array_equal(rec["qs"][t, :K], gq[:K]), (label, t, "codes / act_quant")
        assert np.array_equal(_u32(rec["d"][t, :nd]), _u32(gd[:nd])), (label, t, "d / act_quant")


RECORDS = [(p, 0) for p in PRESETS] + [(17, 1), (18, 1)]


@pytest.mark.parametrize("preset,att_q", RECORDS)
def test_merger_records(device, short_models, preset, att_q):
    g, S = short_models(preset)
    C, mod = S[0], S[0].m
    H, Hk, hd = mod.n_head, mod.n_kv, mod.hd
    p0, nt = 60, 8
    v_off = (H + Hk) * hd

    def zero_v(raw):  # kv head 0's prepared v row exactly 0 (beside a bias: its negative)
        raw = raw.copy()
        raw[v_off:v_off + hd] = 0.0 if mod.layers[0]["bv"] is None else -mod.layers[0]["bv"][:hd].astype(np.float32)
        return raw

    # the prefill pair on [60..67]: plain; kv head 0's V rows all zero; a +- tied maximum
    tie = (np.random.default_rng(3).standard_normal(hd) * 2).astype(np.float16)
    tie[5], tie[6] = 13.25, -13.25
    for case in ("peaked40", "zero_head", "tie"):
        pattern = "dominant" if case == "tie" else "peaked40"
        K, V = (a.copy() for a in C.state(pattern))
        tokens = A.window_tokens(C, pattern, p0, nt)
        if case == "zero_head":
            V[0] = 0
            tokens = [(s, p, zero_v(r)) for s, p, r in tokens]
        if case == "tie":
            t, kr, _ = C.edits("dominant", p0)[-1][1][0]
            K[:, t], V[:, t] = kr, tie
        g.set_kv_rows(0, 0, K, V)
        plain, _ = _launch(g, 0, 0, tokens)
        _restore(g, 0, {0: (K, V)}, tokens)
        att, rec = _launch(g, 0, 0, tokens, att_q=att_q)
        assert att.tobytes() == plain.tobytes(), case
        if case == "zero_head":
            assert not att[:, :mod.G].any() and not rec["qs"][:, :mod.G * hd].any()
            assert not rec["d"][:, :mod.G * hd // (256 if att_q else 32)].any()
        if case == "tie":  # every head's output is the dominant row: both signs of the maximum
            assert (att == np.float32(13.25)).any(axis=2).all() and (att == np.float32(-13.25)).any(axis=2).all()
            assert np.abs(att).max() == 13.25
        _check_records(device, att, rec, att_q, (preset, case))
    # the batched step on three slots; slot 1's kv head 0 all zero
    caches, tokens = A.step_case(S, "peaked40", 3)
    caches[1][1][0] = 0
    tokens[1] = (1, tokens[1][1], zero_v(tokens[1][2]))
    _inject(g, caches)
    plain, _ = _launch(g, 1, 3, tokens)
    _restore(g, 3, caches, tokens)
    att, rec = _launch(g, 1, 3, tokens, att_q=att_q)
    assert att.tobytes() == plain.tobytes()
    assert not att[1, :mod.G].any()
    _check_records(device, att, rec, att_q, (preset, "step"))


# ---------------------------------------------------------------- h: refusals
def test_entry_points_refuse_what_they_cannot_run(device, short_models, synth_llm_path):
    path = synth_llm_path(5)  # (hd 64, G 2): G * hd = 128
    g = m.Llm(device, path, 128)
    C = A.Cases(A.Model(path), n_ctx=128)
    raw = C.raw(3)
    rows = np.zeros((g.n_kv, 2, g.head_dim), np.float16)
    invalid = lambda: pytest.raises(m.HipError, match="rc=-1")
    with invalid():  # no batch state yet
        g.batch_set_kv_rows(0, 0, 0, rows, rows)
    run = lambda mode, slots, pos, seq, **kw: g.debug_attention_multi(0, mode, slots, pos, seq,
                                                                       np.stack([raw] * len(pos)), **kw)
    run(0, 0, [3], [0])
    with invalid():  # slots 0 created none
        g.batch_set_kv_rows(0, 0, 0, rows, rows)
    with invalid():  # seq out of range: the handle's own cache is sequence 0
        run(0, 0, [3], [1])
    with invalid():
        run(0, 2, [3, 4], [0, 2])
    with invalid():  # one token per sequence in the batched step
        run(1, 2, [3, 4], [1, 1])
    with invalid():  # two tokens on one cache row
        run(0, 2, [3, 3], [1, 1])
    with invalid():
        run(0, 0, [128], [0])
    with invalid():
        run(0, 0, [-1], [0])
    with invalid():
        run(0, 0, [3], [0], nt=0)
    with invalid():
        run(0, 0, [3], [0], nt=129)
    with invalid():  # Q8_K records need G * hd a multiple of 256
        run(0, 0, [3], [0], att_q=1)
    with invalid():
        run(0, 0, [3], [0], att_q=2)
    with invalid():  # position 64 lies in the second chunk
        run(0, 0, [3, 64], [0, 0], n_chunks=1)
    with invalid():  # more chunks than the context has
        run(0, 0, [3], [0], n_chunks=3)
    with invalid():
        run(2, 0, [3], [0])
    with invalid():
        run(0, 17, [3], [0])
    with invalid():  # a frozen token in a prefill launch
        run(0, 0, [3], [0], frozen=[1])
    with invalid():
        g.debug_attention_multi(g.n_layer, 0, 0, [3], [0], raw)
    run(0, 2, [3, 4], [0, 1])  # allocates the batch state
    g.batch_set_kv_rows(1, 0, 126, rows, rows)
    for slot, il, p0 in ((2, 0, 0), (-1, 0, 0), (0, g.n_layer, 0), (0, 0, 127), (0, 0, -1)):
        with invalid():
            g.batch_set_kv_rows(slot, il, p0, rows, rows)
    g.close()
    lf = m.Llm(device, synth_llm_path(7), 64)  # tiny lfm2: layer 0 is a short-conv layer
    with invalid():
        lf.debug_attention_multi(0, 0, 0, [3], [0], np.zeros((lf.n_head + 2 * lf.n_kv) * lf.head_dim, np.float32))
    lf.close()
