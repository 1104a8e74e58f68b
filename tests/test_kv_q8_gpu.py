"""GPU: the Q8_0 KV cache (mio_hip_llm_load_kv, kv type 8; csrc/hip/llm_attention_q8.hip), presets 17 (hd 128,
G 2) and 18 (hd 64, G 4) at n_ctx 192. Kernel level: the launches on injected codes / scales and nudged raw rows
against np_attn's float64 attention over the DEQUANTIZED f16 rows under np_attn.bound (the F16 cache's tolerance,
unchanged: the images hold f16 values either way), the appended row bit-equal to np_kv_q8.rows, a masked tail of
codes -128 x scale +Inf. Engine level: prefill == forced steps, queue == generate, logits against the F16 handle
(LOGIT_GAP: measured on the MI355X; asserted 4 x that and not bit-equal), the refusal, MIO_KV_TYPE."""
import os
import subprocess
import sys

import numpy as np
import pytest

import miotts_amd as m
import np_attn as A
import np_kv_q8 as Q

pytestmark = pytest.mark.gpu

N_CTX, C = 192, A.CHUNK
PRESETS, POSITIONS = (17, 18), (0, 31, 32, C - 1, C, 2 * C + 3)
LOGIT_GAP = {17: 0.0346457, 18: 0.0212366}  # measured max |logit difference| to the F16 handle (see docstring)
_cache = {}


@pytest.fixture(scope="module")
def models(device, synth_llm_path):
    def get(preset):
        if preset not in _cache:
            path = synth_llm_path(preset)
            mod = A.Model(path)
            rng = np.random.default_rng(preset)
            state = [tuple(Q.rows((0.5 * rng.standard_normal((mod.n_kv, N_CTX, mod.hd))).astype(np.float16))
                           for _ in "kv") for _ in range(3)]  # [slot] -> (K, V) -> (codes, scales, f16 values)
            _cache[preset] = (m.Llm(device, path, N_CTX, kv_type=8), A.Cases(mod, n_ctx=N_CTX), state)
        return _cache[preset]

    yield get
    for g, _, _ in _cache.values():
        g.close()
    _cache.clear()


def _put(g, st, lo, hi, slot=-1, fill=None):
    """Rows [lo, hi) of a state into layer 0; fill = (code, scale bits): those everywhere instead."""
    (kq, ks, _), (vq, vs, _) = st
    sl = np.s_[:, lo:hi]
    if fill:
        kq = vq = np.full_like(kq, fill[0])
        ks = vs = np.full(ks.shape, fill[1], np.uint16).view(np.float16)
    if hi > lo:
        g.set_kv_rows_q8(0, lo, kq[sl], ks[sl], vq[sl], vs[sl], slot=slot)


def _reference(mod, states, tokens):
    """tokens [(seq, pos, raw)] -> (att, bound [nt, H, hd], [(K (codes, scales), V (..))] per token):
    every token's quantized row replaces row pos of its sequence, then token t attends rows 0..pos."""
    prep = [mod.prepare(0, raw, pos) for _, pos, raw in tokens]
    rows = [(Q.rows(k), Q.rows(v)) for _, k, v in prep]
    KV = {s: [states[s][j][2].astype(np.float64) for j in (0, 1)] for s in {s for s, _, _ in tokens}}
    for (s, pos, _), (rk, rv) in zip(tokens, rows):
        KV[s][0][:, pos], KV[s][1][:, pos] = rk[2], rv[2]
    att, bnd = np.empty((len(tokens), mod.n_head, mod.hd)), np.empty((len(tokens), mod.n_head, mod.hd))
    for t, ((s, pos, _), (q, _, _)) in enumerate(zip(tokens, prep)):
        for h in range(mod.n_head):
            Kh, Vh = KV[s][0][h // mod.G, :pos + 1], KV[s][1][h // mod.G, :pos + 1]
            att[t, h], sc, w = A.attend(q[h], Kh, Vh)
            bnd[t, h] = A.bound(q[h], Kh, Vh, sc, w)
    return att, bnd, rows


def _check_rows(g, tokens, rows, slotted):
    for (s, pos, _), (rk, rv) in zip(tokens, rows):
        kq, ks, vq, vs = g.kv_rows_q8(0, pos + 1, slot=s if slotted else -1)
        for got, want in ((kq, rk[0]), (ks.view(np.uint16), rk[1].view(np.uint16)), (vq, rv[0]),
                          (vs.view(np.uint16), rv[1].view(np.uint16))):
            assert np.array_equal(got[:, pos], want), (s, pos)


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("preset", PRESETS)
def test_decode_attention(models, preset, pos):
    g, cases, state = models(preset)
    raw = cases.raw(pos)
    ref, bnd, rows = _reference(cases.m, state, [(0, pos, raw)])
    _put(g, state[0], 0, pos)
    _put(g, state[0], pos, N_CTX, fill=(-128, 0x7C00))  # masked tail: codes -128 x scale +Inf
    poisoned = g.debug_attention(0, pos, 1, raw)
    _put(g, state[0], pos, N_CTX)
    att = g.debug_attention(0, pos, 1, raw)
    assert att.tobytes() == poisoned.tobytes() and np.isfinite(att).all()
    _check_rows(g, [(0, pos, raw)], rows, False)
    ratio = np.abs(att - ref[0]) / bnd[0]
    print(f"k_attention_q8 preset {preset} pos {pos}: worst err/bound {ratio.max():.3g}")
    assert ratio.max() <= 1.0
    for refused in (lambda: g.kv_rows(0, 1), lambda: g.debug_attention(0, pos, 10, raw)):  # f16 entry, fused launch
        with pytest.raises(m.HipError, match="rc=-6"):
            refused()


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("preset", PRESETS)
def test_multi_token_attention(models, preset, mode):  # 0: 5 tokens of 2 sequences; 1: 3 slots, slot 1 frozen
    g, cases, state = models(preset)
    spots = [(0, C - 2), (1, 3), (0, C - 1), (1, 4), (0, C)] if mode == 0 else [(0, 2 * C + 3), (1, 31), (2, C)]
    tokens = [(s, p, cases.raw(p)) for s, p in spots]
    frozen = None if mode == 0 else [0, 1, 0]
    g.debug_attention_multi(0, 1, 3, [0], [0], tokens[0][2])  # the batch state of 3 slots
    for s in range(3):
        _put(g, state[s], 0, N_CTX, slot=s)
    live = [t for i, t in enumerate(tokens) if not (frozen and frozen[i])]
    ref, bnd, rows = _reference(cases.m, state, live)
    att, _, tickets = g.debug_attention_multi(0, mode, 3, [p for _, p, _ in tokens], [s for s, _, _ in tokens],
                                              np.stack([r for _, _, r in tokens]), frozen=frozen)
    assert not tickets.any()
    _check_rows(g, live, rows, True)
    if frozen:  # no output, no cache row
        assert (att[1].view(np.uint32) == 0x7FC5A5A5).all()
        assert np.array_equal(g.kv_rows_q8(0, N_CTX, slot=1)[0], state[1][0][0])
        att = att[[0, 2]]
    ratio = np.abs(att - ref) / bnd
    print(f"multi-token q8 attention preset {preset} mode {mode}: worst err/bound {ratio.max():.3g}")
    assert np.isfinite(att).all() and ratio.max() <= 1.0


def _planes(g, n, slot=-1):
    return [a.tobytes() for il in range(g.n_layer) for a in g.kv_rows_q8(il, n, slot=slot)]


@pytest.mark.parametrize("n", (C - 1, C + 1, 2 * C + 2))
@pytest.mark.parametrize("preset", PRESETS)
def test_prefill_equals_forced_steps(models, preset, n):
    g = models(preset)[0]
    toks = (np.arange(n) * 7919 + preset) % g.n_vocab
    lp, pp = g.prefill(toks), _planes(g, n)
    for p, t in enumerate(toks):
        le = g.eval(int(t), p)
    assert lp.tobytes() == le.tobytes() and pp == _planes(g, n)


@pytest.mark.parametrize("preset", PRESETS)
def test_queue_equals_generate(models, preset):
    g = models(preset)[0]
    prompts = [list((np.arange(5 + 3 * u) * 31 + u) % g.n_vocab) for u in range(4)]
    seeds = [11, 12, 13, 14]
    outs, stats = g.generate_queue(prompts, 9, 0.8, seeds, slots=3)  # 4 utterances on 3 slots: one refill
    assert stats["refills"] == 1
    for u in range(4):
        assert np.array_equal(outs[u], g.generate(prompts[u], 9, 0.8, seeds[u])), u
    # utterance 3 ran last on the single stream and in its slot
    n = len(prompts[3]) + 9 - 1
    assert _planes(g, n) == _planes(g, n, slot=stats["slot_of"][3])
    batch = g.generate_batch(prompts[:3], 9, 0.8, seeds[:3])
    assert all(np.array_equal(batch[u], outs[u]) for u in range(3))


@pytest.mark.parametrize("preset", PRESETS)
def test_logits_against_the_f16_handle(device, models, synth_llm_path, preset):
    g = models(preset)[0]
    f = m.Llm(device, synth_llm_path(preset), N_CTX)
    toks = (np.arange(40) * 104729 + 3) % g.n_vocab
    gap, same = 0.0, True
    for p, t in enumerate(toks):
        a, b = g.eval(int(t), p), f.eval(int(t), p)
        gap, same = max(gap, float(np.abs(a - b).max())), same and a.tobytes() == b.tobytes()
    f.close()
    print(f"q8_0 vs f16 cache, preset {preset}: max |logit difference| {gap:.6g}")
    assert not same and gap <= 4 * LOGIT_GAP[preset]


def test_kv_type_selection(device, synth_llm_path):
    path = synth_llm_path(18)
    with pytest.raises(m.HipError, match="q4_0"):
        m.Llm(device, path, 64, kv_type=2)
    code = ("import miotts_amd as m; d = m.Device(0); "
            f"print(m.Llm(d, {path!r}, 64).kv_type(), m.Llm(d, {path!r}, 64, kv_type=1).kv_type())")
    env = dict(os.environ, MIO_KV_TYPE="q8_0", PYTHONPATH=os.path.dirname(os.path.dirname(m.__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["8", "1"]
