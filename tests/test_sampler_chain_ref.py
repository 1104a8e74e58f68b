"""CPU: the numpy reference of the sampler chain (tests/np_sampler_chain.py) on hand-computed cases,
against np_sampler where the chain is neutral, and the teeth of the shared case lists: every mutant
(a defective restatement of the chain) is rejected by at least one case the GPU tests run, and the
reference alone keeps every case list under the ambiguity cap.

A mutant is rejected by a kernel-level case when what a correct kernel returns there (the
reference's penalised row, kept count, cut id and token) fails the checks of
test_sampler_chain_gpu.py made against the mutant. The prompt-as-history mutant cannot show through
the one-launch entry (it has no prompt); it is rejected by the narrow end-to-end case, run here on
seeded rows in place of the model's logits, through the compare_run the GPU test uses.
"""
import numpy as np
import pytest

import np_sampler as S
import np_sampler_chain as C


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _row(vals, n=16, fill=-50.0):
    r = np.full(n, fill, np.float32)
    r[:len(vals)] = vals
    return r


def test_hand_penalties():
    row = np.array([2.0, -2.0, 0.5, 0.0, 1.0, 3.0], np.float32)
    P = C.params(repeat_penalty=2.0, frequency_penalty=0.25, presence_penalty=0.5, repeat_last_n=4)
    #   history, last 4: [1, 0, 0, 3] -> id 0 twice, id 1 once, id 3 once; id 4 (older) is out
    out = C.penalise(row, [4, 4, 1, 0, 0, 3], P, 0, 6)
    #   id 0: 2 / 2 = 1, - (2 * .25 + .5) = 0;  id 1: -2 * 2 = -4, - .75 = -4.75;  id 3: 0 * 2 = 0, - .75
    assert out.tolist() == [0.0, -4.75, 0.5, -0.75, 1.0, 3.0]
    # a history shorter than repeat_last_n counts whole
    out = C.penalise(row, [0, 0, 1], P._replace(repeat_last_n=5), 0, 6)
    assert out.tolist() == [0.0, -4.75, 0.5, 0.0, 1.0, 3.0]
    # ids outside the window keep their bits
    out = C.penalise(row, [0, 5], P, 1, 5)
    assert np.array_equal(_bits(out), _bits(row))
    # repeat_last_n 0: no penalties
    assert np.array_equal(_bits(C.penalise(row, [0, 1], P._replace(repeat_last_n=0), 0, 6)), _bits(row))
    # f32 rounding of each step: 1 / 3 is rounded before the subtraction
    P3 = C.params(repeat_penalty=3.0, frequency_penalty=0.1)
    want = np.float32(np.float32(np.float32(1.0) / np.float32(3.0)) - np.float32(np.float32(1.0) * np.float32(0.1)))
    assert _bits(C.penalise(np.array([1.0], np.float32), [0], P3, 0, 1))[0] == _bits(want)[0]


def test_hand_top_k_top_p_min_p():
    # logits ln 4, ln 2, ln 1, ln 1 at ids 3, 1, 0, 2: masses 4 2 1 1 (Z = 8), order 3, 1, 0, 2
    row = _row([0.0, np.log(2.0), 0.0, np.log(4.0)], 4)
    c = C.chain(row, [], C.params(top_k=2), 0.0, 1, 0, 0, 4)
    assert c.order.tolist() == [3, 1, 0, 2] and (c.m_lo, c.m_hi) == (2, 2)
    # top-p: mass before ids 3, 1, 0, 2 is 0, .5, .75, .875 of Z
    for p, kept in ((0.0, 1), (0.3, 1), (0.6, 2), (0.8, 3), (0.9, 4), (1.0, 4)):
        c = C.chain(row, [], C.params(top_p=p), 0.0, 1, 0, 0, 4)
        assert (c.m_lo, c.m_hi) == (kept, kept), (p, c.m_lo, c.m_hi)
    # exactly at the crossing (f32 ln 2 makes the masses inexact): the range holds both
    c = C.chain(row, [], C.params(top_p=0.5), 0.0, 1, 0, 0, 4)
    assert c.m_lo <= 1 and c.m_hi >= 2
    # top-p over the top-k survivors: Z = 6, mass before id 1 is 4/6
    assert C.chain(row, [], C.params(top_k=2, top_p=0.6), 0.0, 1, 0, 0, 4).m_hi == 1
    assert C.chain(row, [], C.params(top_k=2, top_p=0.7), 0.0, 1, 0, 0, 4).m_lo == 2
    # min-p: l >= ln 4 + ln(min_p)
    for mp, kept in ((0.6, 1), (0.4, 2), (0.2, 4), (2.0, 1)):
        c = C.chain(row, [], C.params(min_p=mp), 0.0, 1, 0, 0, 4)
        assert (c.m_lo, c.m_hi) == (kept, kept), (mp, c.m_lo, c.m_hi)
    # all-equal rows are exact: n = 64, p = .5 keeps 32, p = .3 keeps 20 (the crossing id stays)
    eq = np.full(64, -1.5, np.float32)
    for p, kept in ((0.5, 32), (0.3, 20)):
        c = C.chain(eq, [], C.params(top_p=p), 0.8, 1, 0, 0, 64)
        assert (c.m_lo, c.m_hi) == (kept, kept) and c.order[:kept].tolist() == list(range(kept))
    # T <= 0 with penalties: the argmax of the penalised row
    row = _row([5.0, 4.0, 1.0], 3)
    assert C.sample(row, [0], C.params(presence_penalty=2.0), 0.0, 1, 3, 0, 3) == 1
    assert C.sample(row, [], C.NEUTRAL, 0.8, 1, 3, 2, 2) == 2  # empty window
    assert C.sample(row, [], C.NEUTRAL, 0.8, 1, 3, 0, 3, forced=1) == 1


def test_neutral_is_np_sampler():
    rng = np.random.default_rng(1)
    for i in range(60):
        row = C.family_row(C.FAMILIES[i % 3], rng, 2000)
        lo = int(rng.integers(0, 1500))
        hi = lo + int(rng.integers(1, 500))
        T = (0.8, 0.0, 5.0)[i % 3]
        hist = rng.integers(lo, hi, 10).tolist()
        for P in (C.NEUTRAL, C.params(repeat_last_n=0, repeat_penalty=1.0), C.params(top_k=hi - lo)):
            assert C.sample(row, hist, P, T, 42 + i, i, lo, hi) == S.sample(row, T, 42 + i, i, lo, hi).winner


def test_top_k_1_is_argmax_at_any_T():
    rng = np.random.default_rng(2)
    for i in range(40):
        row = C.family_row(C.FAMILIES[i % 3], rng, 3000)
        lo, hi = 100, 100 + (1, 2, 65, 2900)[i % 4]
        for T in (0.0, 0.05, 0.8, 5.0):
            assert C.sample(row, [], C.params(top_k=1), T, 679, i, lo, hi) == lo + int(np.argmax(row[lo:hi]))


def _rejects(case, mutant) -> bool:
    """Would the GPU test, made against the mutant, fail on a correct kernel's result?"""
    ref, mut = C.run_case(case), C.run_case(case, mutant)
    if not np.array_equal(_bits(ref.row), _bits(mut.row)):
        return True
    if ref.m_lo > mut.m_hi or ref.m_hi < mut.m_lo:
        return True
    if ref.m_lo == ref.m_hi and ref.order[ref.m_lo - 1] != mut.order[ref.m_lo - 1]:
        return True
    return not C.accept(ref.winners[0], mut, case["lo"], case["T"]).ok


@pytest.mark.parametrize("mutant", [x for x in C.MUTANTS if x != "prompt_as_history"])
def test_mutants_rejected_by_kernel_cases(mutant):
    cases = C.exact_cases() + C.ranged_cases()
    hits = [c["name"] for c in cases if _rejects(c, mutant)]
    print(mutant, "rejected by", len(hits), "cases, e.g.", hits[:3])
    assert hits, mutant


def _synthetic_run(n_tokens=C.E2E_TOKENS, seed=31):
    """The narrow end-to-end case on seeded N(0, 1) rows: (prompt, rows, the reference's tokens)."""
    N = C.NARROW
    lo, hi = N["allow"]
    rng = np.random.default_rng(seed)
    prompt = C.narrow_prompt()
    rows, toks = [], []
    for i in range(n_tokens):
        rows.append(C.family_row("n1", rng))
        toks.append(C.sample(rows[-1], toks, N["P"], N["T"], N["seed"], len(prompt) - 1 + i, lo, hi))
    return prompt, rows, toks


def test_prompt_as_history_rejected_by_narrow_run():
    N = C.NARROW
    lo, hi = N["allow"]
    prompt, rows, toks = _synthetic_run()
    assert len(set(toks)) < len(toks), "no id came back: the penalties are not exercised"
    args = (toks, rows, N["P"], N["T"], N["seed"], len(prompt) - 1, lo, hi)
    bad, near, amb = C.compare_run(*args, prompt=prompt)
    assert not bad and near <= S.CAP * len(toks) and amb == 0
    bad, _, _ = C.compare_run(*args, prompt=prompt, mutant="prompt_as_history")
    assert bad, "the prompt-as-history mutant passes the narrow run"


@pytest.mark.parametrize("name, cases", [("exact", C.exact_cases), ("ranged", C.ranged_cases),
                                         ("neutral", C.neutral_cases), ("wide exact", C.wide_exact_cases),
                                         ("wide ranged", C.wide_ranged_cases),
                                         ("wide neutral", C.wide_neutral_cases)])
def test_ambiguity_cap_of_the_case_lists(name, cases):
    """Per case list: ambiguous steps (the admissible prefixes disagree on the winner) at most CAP of
    the steps; an exact list has none and its ranges are single counts."""
    cs = cases()
    amb = 0
    for c in cs:
        r = C.run_case(c)
        amb += r.ambiguous
        if c["exact"]:
            assert r.m_lo == r.m_hi and not r.ambiguous, c["name"]
    print(name, len(cs), "cases,", amb, "ambiguous")
    assert amb <= S.CAP * len(cs), (name, amb, len(cs))


def test_wide_cases_take_the_wide_body():
    """Every wide case has a window past the register-resident limit, one of them just past it, and
    wave segments (a sixteenth of the window, rounded up to 64) that are no multiple of the wide
    body's 256-id load stride; the mutants with a kernel-level case are rejected there too."""
    cs = C.wide_exact_cases() + C.wide_ranged_cases() + C.wide_neutral_cases()
    widths = {c["hi"] - c["lo"] for c in cs}
    assert min(widths) == C.REG_LIMIT + 1 and max(widths) == C.WIDE_VOCAB
    seg = {((w + 15) // 16 + 63) // 64 * 64 for w in widths}
    assert any(s % 256 for s in seg) and any(s % 256 == 0 for s in seg)
    assert any(w % 64 for w in widths)
    for mutant in ("p_cross_excluded", "topk_ties_highest", "penalty_swap", "no_count", "long_history", "minp_vs_sum"):
        assert any(_rejects(c, mutant) for c in cs), mutant


def test_reported_kept_count_binds_the_token():
    """With the kernel's own kept count the token must win THAT prefix: the winner of another
    admissible prefix is rejected."""
    # masses 4 2 1 1 at ids 3 1 0 2 and p = .5: the crossing is inexact in f32, the range holds 1 and
    # 2 ids; a seed at which id 1's draw beats id 3's makes the two prefixes disagree
    row = _row([0.0, np.log(2.0), 0.0, np.log(4.0)], 4)
    r = next(c for c in (C.chain(row, [], C.params(top_p=0.5), 0.8, seed, 3, 0, 4) for seed in range(200))
             if c.ambiguous)
    assert (r.m_lo, r.m_hi) == (1, 2) and r.winners == [3, 1]
    w_lo, w_hi = r.winners[0], r.winners[-1]
    assert C.accept(w_hi, r, 0, 0.8).ok and C.accept(w_lo, r, 0, 0.8, kept=r.m_lo).ok
    assert not C.accept(w_hi, r, 0, 0.8, kept=r.m_lo).ok
    assert not C.accept(w_lo, r, 0, 0.8, kept=r.m_hi + 1).ok


def test_ranged_cases_are_informative():
    """The ranges are tight enough to mean something: most top-p / min-p cases pin the kept count to
    a handful of ids (the wide flat rows are the exception the range exists for)."""
    cs = C.ranged_cases()
    spans = np.array([(lambda r: r.m_hi - r.m_lo)(C.run_case(c)) for c in cs])
    print("range widths: median", np.median(spans), "max", spans.max())
    assert np.median(spans) <= 2
