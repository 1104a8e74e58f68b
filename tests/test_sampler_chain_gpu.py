"""GPU parity of the sampler chain (k_sample_chain) against tests/np_sampler_chain.py.

Kernel level, through mio_hip_llm_debug_sample_chain (one launch of the chain kernel + the flush
sampler on an injected row of the tiny preset's 13,312-id vocabulary): the case lists of
np_sampler_chain. An exact case must return the reference's kept count, cut id and, bit for bit,
penalised row; a ranged case a kept count inside [m_lo, m_hi] with the cut id that count implies;
every token must pass np_sampler_chain.accept as the winner of the prefix the kernel reported.
Ambiguous steps and near-ties are capped per list. The same kinds of cases run on the 0.1B shape's
61,952-id vocabulary at windows past 13 * 1024 ids, where the kernel takes its other body (the row
re-read from memory by every pass instead of kept in registers), with a replayed generate and a
batch over the whole vocabulary.

End to end: the replay scheme of test_sampler_gpu.py (teacher-forced eval of prompt + tokens gives
the logits every step sampled from) with the run's own earlier tokens as history; generate_batch
against generate with the chain on; and the neutral settings against a handle that never heard of
the chain (tokens, step_kinds, steps_issued). The teeth are in test_sampler_chain_ref.py.
"""
import numpy as np
import pytest

import miotts_amd as m
import np_sampler as S
import np_sampler_chain as C

pytestmark = pytest.mark.gpu

N_CTX = 512  # a history of 300 tokens in front of the step


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sampling(P):
    return m.Sampling(**P._asdict())


@pytest.fixture(scope="module")
def tiny(device, synth_llm_path):
    g = m.Llm(device, synth_llm_path(0), N_CTX)
    assert g.n_vocab == C.N_VOCAB
    yield g
    g.close()


def _check_list(g, cases, exact):
    near = amb = 0
    for c in cases:
        ref = C.run_case(c)
        tok, kept, cut, pen = g.debug_sample_chain(c["row"], c["history"], _sampling(c["P"]), c["T"], c["seed"],
                                                   c["step"], c["lo"], c["hi"], penalised=True)
        what = (c["name"], tok, kept, cut, ref.m_lo, ref.m_hi)
        assert np.array_equal(_bits(pen), _bits(ref.row)), ("penalised row", c["name"])
        if exact:
            assert ref.m_lo == ref.m_hi == kept, what
        assert ref.m_lo <= kept <= ref.m_hi, what
        assert cut == ref.order[kept - 1], what + (int(ref.order[kept - 1]),)
        v = C.accept(tok, ref, c["lo"], c["T"], kept=kept)  # the winner of the prefix the kernel reported
        assert v.ok, what + (ref.winners,)
        near += v.near_tie
        amb += v.ambiguous
    print(len(cases), "cases:", near, "near-ties,", amb, "ambiguous")
    assert near <= S.CAP * len(cases) and amb <= S.CAP * len(cases)


def test_exact_cases(tiny):
    """top-k alone on random and all-equal rows at every width and offset, top-p on all-equal rows
    (n = 64: p = .5 keeps 32, p = .3 keeps 20), rows with -inf, histories with repeats, ids outside
    the window and lengths 0, 1, 64, 256 and longer than repeat_last_n."""
    _check_list(tiny, C.exact_cases(), True)


def test_ranged_cases(tiny):
    """top-p in {1e-6, .5, .9, .999999}, min-p in {.05, .5, 1} on N(0, 1), N(0, 4) and Zipf-like rows
    at every width and offset, and all knobs together."""
    _check_list(tiny, C.ranged_cases(), False)


def test_neutral_parameters_return_np_sampler_token(tiny):
    """The launch with every knob neutral keeps every id and draws np_sampler.sample's token (the
    history present, but no penalty on)."""
    near = 0
    for c in C.neutral_cases():
        tok, kept, cut, pen = tiny.debug_sample_chain(c["row"], c["history"], _sampling(c["P"]), c["T"], c["seed"],
                                                      c["step"], c["lo"], c["hi"], penalised=True)
        p = S.sample(c["row"], c["T"], c["seed"], c["step"], c["lo"], c["hi"])
        assert S.accepted(tok, p), (c["name"], tok, p)
        assert kept == c["hi"] - c["lo"] and np.array_equal(_bits(pen), _bits(c["row"])), c["name"]
        near += p.near_tie
    assert near <= S.CAP * len(C.neutral_cases())
    # the empty window: the launch leaves the step alone, the token is lo
    c = C.neutral_cases()[0]
    assert tiny.debug_sample_chain(c["row"], [], _sampling(C.params(top_k=5)), 0.8, 42, 7, 777, 777) == (777, 0, -1)


# ---------------------------------------------------------------- windows past the register limit
@pytest.fixture(scope="module")
def wide(device, synth_llm_path):
    g = m.Llm(device, synth_llm_path(C.WIDE_PRESET), N_CTX)
    assert g.n_vocab == C.WIDE_VOCAB > C.REG_LIMIT
    yield g
    g.close()


def test_wide_exact_cases(wide):
    """Windows wider than 13 * 1024 ids take the kernel's other body (the row re-read from memory by
    every pass): top-k on random and all-equal rows, all-equal top-p, -inf rows and histories, at
    13,313 ids, at widths whose wave segments are no multiple of the load stride, and over the
    whole 61,952-id vocabulary."""
    _check_list(wide, C.wide_exact_cases(), True)


def test_wide_ranged_and_neutral_cases(wide):
    _check_list(wide, C.wide_ranged_cases(), False)
    for c in C.wide_neutral_cases():
        tok, kept, cut, pen = wide.debug_sample_chain(c["row"], c["history"], _sampling(c["P"]), c["T"], c["seed"],
                                                      c["step"], c["lo"], c["hi"], penalised=True)
        p = S.sample(c["row"], c["T"], c["seed"], c["step"], c["lo"], c["hi"])
        assert S.accepted(tok, p) and not p.near_tie, (c["name"], tok, p)
        assert kept == c["hi"] - c["lo"] and np.array_equal(_bits(pen), _bits(c["row"])), c["name"]


def test_wide_generate_replay(wide):
    """Replayed generates over the whole vocabulary of the wide model (the window real use has
    without a speech-only harness), every knob on, T 0.8 and T 0, and the batch against generate."""
    P = C.E2E_CONFIGS[3][1]
    tally = [0, 0, 0]
    for T, plen in ((0.8, 5), (0.0, 140)):
        toks, (bad, near, amb) = _run(wide, S.prompt(plen), C.E2E_TOKENS, P, T, S.SEEDS[1], (-1, -1))
        assert not bad, (T, plen, bad[:3])
        tally = [tally[0] + near, tally[1] + amb, tally[2] + len(toks)]
    print("(near-ties, ambiguous, steps):", tally)
    assert tally[0] <= S.CAP * tally[2] and tally[1] <= S.CAP * tally[2]
    prompts = [S.prompt(n, 50 + b) for b, n in enumerate((5, 1, 33))]
    seeds = [679, (1 << 40) + 679, 42]
    got = wide.generate_batch(prompts, 16, 0.8, seeds, allow=(-1, -1))
    for b in range(3):
        one = wide.generate(prompts[b], 16, 0.8, seeds[b], allow=(-1, -1))
        assert np.array_equal(np.asarray(got[b]), one), (b, got[b], one)
    wide.set_sampling()


def test_invalid_settings_are_refused(tiny):
    before = tiny.get_sampling()
    for bad in (dict(repeat_penalty=0.0), dict(repeat_penalty=-1.0), dict(top_p=float("nan")),
                dict(min_p=float("nan")), dict(repeat_last_n=-1), dict(repeat_last_n=257),
                dict(frequency_penalty=float("nan"))):
        with pytest.raises(m.HipError, match="rc=-1"):
            tiny.set_sampling(**bad)
    assert tiny.get_sampling() == before == m.Sampling().as_dict()
    tiny.set_sampling(top_k=40, top_p=0.5, repeat_last_n=256)
    got = tiny.get_sampling()
    assert got["top_k"] == 40 and got["top_p"] == 0.5 and got["repeat_last_n"] == 256
    tiny.set_sampling()
    assert tiny.get_sampling() == before


# ---------------------------------------------------------------- end to end
def _replay(g, prompt, toks):
    seq = [int(t) for t in prompt] + [int(t) for t in toks[:-1]]
    P = len(prompt) - 1
    return [lg for pos, lg in ((pos, g.eval(t, pos)) for pos, t in enumerate(seq)) if pos >= P]


def _run(g, prompt, n, P, T, seed, allow):
    g.set_sampling(_sampling(P))
    toks = g.generate(prompt, n, T, seed, allow=allow)
    last = g.logits()
    assert len(toks) == n
    rows = _replay(g, prompt, toks)  # eval never runs the chain
    assert np.array_equal(_bits(last), _bits(rows[-1])), "the chain left the logits row changed"
    lo, hi = S.window(allow, g.n_vocab)
    return toks, C.compare_run(toks, rows, P, T, seed, len(prompt) - 1, lo, hi, prompt=prompt)


@pytest.mark.parametrize("preset", [0, 1, 11])
def test_generate_replay(device, synth_llm_path, preset):
    """Four chain configurations, two prompt lengths, T 0.8 and T 0 over the speech window, and the
    narrow case (65 ids, a history of 16, a prompt of the window's own ids: sampled ids come back and
    the prompt must not count). Every token against the reference on the replayed logits."""
    g = m.Llm(device, synth_llm_path(preset), N_CTX)
    tally = {}
    for ci, (name, P) in enumerate(C.E2E_CONFIGS):
        for pi, plen in enumerate(C.E2E_PROMPT_LENS):
            for T in C.E2E_TEMPS:
                toks, (bad, near, amb) = _run(g, S.prompt(plen), C.E2E_TOKENS, P, T, S.SEEDS[(ci + pi) % 3], S.SPEECH)
                assert not bad, (name, plen, T, bad[:3])
                assert ((toks >= S.SPEECH[0]) & (toks < S.SPEECH[1])).all()
                a = tally.setdefault(name, [0, 0, 0])
                a[0] += near
                a[1] += amb
                a[2] += len(toks)
    N = C.NARROW
    toks, (bad, near, amb) = _run(g, C.narrow_prompt(), C.E2E_TOKENS, N["P"], N["T"], N["seed"], N["allow"])
    assert not bad, ("narrow", bad[:3])
    assert len(set(toks.tolist())) < len(toks), "no id came back: the penalties were not exercised"
    tally["narrow"] = [near, amb, len(toks)]
    print("(near-ties, ambiguous, steps) per configuration:", tally)
    over = {k: v for k, v in tally.items() if v[0] > S.CAP * v[2] or v[1] > S.CAP * v[2]}
    assert not over, over
    g.close()


def test_batch_equals_generate(tiny):
    """generate_batch with the chain on (B = 3 and 9, ragged prompts, per-stream seeds): each stream
    has its own history and returns exactly generate's tokens."""
    lens = (5, 1, 140, 9, 33, 2, 64, 17, 100)
    seeds = (679, (1 << 40) + 679, 42, 2199, 706, 7, (1 << 63) + 1, 1000, 1001)
    N = C.NARROW
    for name, P, T, allow in (("all", C.E2E_CONFIGS[3][1], 0.8, S.SPEECH), ("narrow", N["P"], N["T"], N["allow"]),
                              ("minp+rep T0", C.E2E_CONFIGS[2][1], 0.0, S.SPEECH)):
        tiny.set_sampling(_sampling(P))
        for B in (3, 9):
            prompts = [S.prompt(n, 50 + b) for b, n in enumerate(lens[:B])]
            got = tiny.generate_batch(prompts, 24, T, list(seeds[:B]), allow=allow)
            for b in range(B):
                one = tiny.generate(prompts[b], 24, T, seeds[b], allow=allow)
                assert np.array_equal(np.asarray(got[b]), one), (name, B, b, got[b], one)
    tiny.set_sampling()


def test_neutral_settings_change_nothing(device, synth_llm_path):
    """Neutral set_sampling and set_sampling(NULL) give the tokens, step_kinds and steps_issued of a
    handle that never called it; with a knob on, step_kinds has exactly one more entry, kind 14, and
    turning it off again gives the first tokens back."""
    path = synth_llm_path(0)
    p = S.prompt(5)
    g0 = m.Llm(device, path, N_CTX)
    want = g0.generate(p, 40, 0.8, 679, allow=S.SPEECH)
    kinds0, issued0 = g0.step_kinds(), g0.steps_issued()
    wb = g0.generate_batch([p, S.prompt(9)], 16, 0.8, [679, 42], allow=S.SPEECH)
    g = m.Llm(device, path, N_CTX)
    for setter in (lambda: g.set_sampling(m.Sampling()), lambda: g.set_sampling(),
                   lambda: g.set_sampling(repeat_last_n=0)):
        setter()
        assert np.array_equal(g.generate(p, 40, 0.8, 679, allow=S.SPEECH), want)
        assert g.step_kinds() == kinds0 and g.steps_issued() == issued0
    g.set_sampling(top_k=40)
    kinds1 = g.step_kinds()
    assert kinds1 == kinds0 + [14] and m.STEP_KIND_NAMES[14] == "sample_chain"
    # the diagnostics run the plain step: 14 is refused, the timeline has the plain launch count
    with pytest.raises(m.HipError, match="rc=-1"):
        g.time_kernel(14, 2)
    on = g.generate(p, 40, 0.8, 679, allow=S.SPEECH)
    assert len(on) == 40 and g.steps_issued() == issued0
    g.set_sampling()
    assert g.step_kinds() == kinds0
    assert np.array_equal(g.generate(p, 40, 0.8, 679, allow=S.SPEECH), want)
    got = g.generate_batch([p, S.prompt(9)], 16, 0.8, [679, 42], allow=S.SPEECH)
    assert all(np.array_equal(a, b) for a, b in zip(got, wb))
    # a chain that keeps everything (top_k = the window) draws the plain sampler's tokens, through
    # the chain launch
    g.set_sampling(top_k=12799, repeat_penalty=1.0)
    g.set_sampling(min_p=1e-30)
    assert g.step_kinds() == kinds0 + [14]
    assert np.array_equal(g.generate(p, 40, 0.8, 679, allow=S.SPEECH), want)
    g.close()
    g0.close()
