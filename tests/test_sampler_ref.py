"""CPU: the numpy sampler reference (tests/np_sampler.py) against the C oracle's mo_sample /
mo_gumbel, the finiteness of the Gumbel noise over every draw, and the teeth of
tests/test_sampler_gpu.py.

Teeth: each mutant of the reference below, run on synthetic logits at a case of the GPU test
(same windows, temperatures, seeds, prompt lengths and tie block), must produce a token the
acceptance rule rejects there: a kernel with that defect would fail the GPU test at that case.

  mutant                                       case
  step frozen at 0                             T 0.8, speech window, prompt of 5
  step counted from the first generated token  T 0.8, speech window, prompts of 5 and 140
  id taken relative to lo                      T 0.8, speech window (lo 260)
  seed_hi dropped                              seed (1 << 40) + 679
  ties to the highest id                       tie block, T 0, windows inside it
  hi inclusive                                 narrow windows, T 0 and T 0.8
  v * T instead of v / T                       T 0.05 and T 5, speech window
  noise added at T <= 0                        tie block, T 0
"""
import numpy as np
import pytest

import np_sampler as S
import pyoracle

N_VOCAB = 13312  # the tiny presets' vocabulary
TIE_A, TIE_N = S.TIE_A, S.TIE_N  # the tie block of test_sampler_gpu.py


def _logits(n_steps, seed=11, tie=False):
    lg = np.random.default_rng(seed).standard_normal((n_steps, N_VOCAB)).astype(np.float32)
    if tie:
        lg[:, TIE_A:TIE_A + TIE_N] = lg[:, TIE_A:TIE_A + 1]
    return lg


def test_draw_examples():
    """The draws named in DESIGN.md: h >> 40 == 2^24 - 1 at ids inside the speech window, and the
    first such draw of seed 42 among ids < 13312."""
    for seed, step, idx in ((679, 6, 4872), (2199, 4, 6328), (706, 5, 10581), (42, 825, 5435)):
        assert int(S.draw(seed, step, [idx])[0]) == (1 << 24) - 1, (seed, step, idx)
    ids = np.arange(N_VOCAB)
    M = (1 << 64) - 1

    def mix(x):  # the hash in Python integers
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    for seed, step, idx in ((42, 7, 9), ((1 << 63) + 5, (1 << 31) - 1, 164735)):
        assert int(S.draw(seed, step, [idx])[0]) == mix(seed ^ mix((step << 32) | idx)) >> 40
    assert not any(((S.draw(42, s, ids) == (1 << 24) - 1).any()) for s in range(825))
    assert np.flatnonzero(S.draw(42, 825, ids) == (1 << 24) - 1).tolist() == [5435]


def test_every_draw_gives_finite_monotone_noise():
    """All 2^24 values of h >> 40: u < 1, the noise finite and non-decreasing in the draw, in
    float64 and in f32 arithmetic; without the clamp exactly one value (2^24 - 1) is infinite, and
    the clamp changes no other u."""
    d = np.arange(1 << 24, dtype=np.uint64)
    u = S.u_of_draw(d)
    assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
    g = S.noise_of_u(u)
    assert np.isfinite(g).all() and (np.diff(g) >= 0).all()
    g32 = -np.log(-np.log(u))
    assert g32.dtype == np.float32 and np.isfinite(g32).all() and (np.diff(g32) >= 0).all()
    raw = S.u_of_draw(d, clamp=False)
    changed = np.flatnonzero(raw != u)
    assert changed.tolist() == [(1 << 24) - 1] and raw[-1] == 1.0
    assert np.isposinf(S.noise_of_u(raw[-1:])[0])


@pytest.mark.parametrize("seed,step,idx", [(679, 6, 4872), (2199, 4, 6328), (706, 5, 10581)])
def test_oracle_noise_finite_at_the_largest_draw(seed, step, idx):
    g = float(pyoracle.oracle().mo_gumbel(seed, step, idx))
    want = float(S.noise(seed, step, [idx])[0])
    assert np.isfinite(g) and abs(g - want) <= S.err(0.0, want), (g, want)


def test_oracle_noise_matches():
    """mo_gumbel (f32, glibc logf) within the derived bound of the float64 noise; 64-bit seeds and
    large steps and ids included."""
    rng = np.random.default_rng(2)
    o = pyoracle.oracle()
    for _ in range(2000):
        seed = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        step, idx = int(rng.integers(0, 1 << 20)), int(rng.integers(0, 200000))
        want = float(S.noise(seed, step, [idx])[0])
        got = float(o.mo_gumbel(seed, step, idx))
        assert abs(got - want) <= S.err(0.0, want), (seed, step, idx, got, want)


@pytest.mark.parametrize("T", [0.0, 0.05, 0.8, 5.0])
@pytest.mark.parametrize("width", [1, 2, 64, 65, 12800])
def test_reference_matches_oracle(T, width):
    """np_sampler.sample == pyoracle.sample outside near-ties, on random logits, with the window at
    both ends of the vocabulary; near-ties within the cap."""
    n = 60
    lg = _logits(n, seed=width)
    bad, near, steps = [], 0, 0
    for lo in (0, N_VOCAB - width):
        for seed in (42, (1 << 40) + 679):
            got = [pyoracle.sample(lg[i], T, seed, 7 + i, lo, lo + width) for i in range(n)]
            b, k = S.compare(got, lg, T, seed, 7, lo, lo + width)
            bad += b
            near += k
            steps += n
    print(f"T={T} width={width}: {near} near-ties in {steps} steps")
    assert not bad, bad[:3]
    assert near <= S.CAP * steps
    if T <= 0 or width == 1:
        assert near == 0


def test_reference_edges():
    lg = _logits(1)[0]
    assert S.sample(lg, 0.8, 42, 3, 500, 500).winner == 500            # empty window -> lo
    assert S.sample(lg, 0.8, 42, 3, 500, 400).winner == 500
    assert S.sample(lg, 0.8, 42, 3, 0, N_VOCAB, forced=77).winner == 77
    assert S.sample(lg, 0.8, 42, 3, 0, N_VOCAB, forced=-1).winner == S.sample(lg, 0.8, 42, 3, 0, N_VOCAB).winner
    assert S.window((-1, -1), N_VOCAB) == (0, N_VOCAB) and S.window((0, N_VOCAB + 1000), N_VOCAB) == (0, N_VOCAB)
    # T = 1e-30: v / T is finite in f32 (about 1e30 v) and absorbs the noise: the largest logit wins
    p = S.sample(lg, 1e-30, 42, 3, 260, 13060)
    assert p.winner == 260 + int(np.argmax(lg[260:13060])) and not p.near_tie
    # T = 1e-45 (a subnormal f32): the quotient overflows, every positive logit ties at +inf, the
    # lowest such id wins, exactly
    p = S.sample(lg, 1e-45, 42, 3, 260, 13060)
    assert np.float32(1e-45) > 0 and p.winner == 260 + int(np.argmax(lg[260:13060] > 0)) and not p.near_tie
    assert p.winner != 260 + int(np.argmax(lg[260:13060]))
    # exact ties at T = 0 go to the lowest id and are no near-tie
    tied = _logits(1, tie=True)[0]
    p = S.sample(tied, 0.0, 42, 3, TIE_A + 5, TIE_A + 70)
    assert p.winner == TIE_A + 5 and p.gap == 0.0 and not p.near_tie


def test_near_tie_share_with_derived_eps():
    """The reference alone stays far inside the cap: 1500 steps of sigma = 1 logits over a
    12 800-id window at T 0.8 and 0.05, near-ties by the derived eps counted (eps itself printed:
    about 2^-15 absolute at T 0.8)."""
    lg = _logits(1500, seed=21)
    for T in (0.8, 0.05):
        picks = [S.sample(lg[i], T, 42, i, *S.SPEECH) for i in range(len(lg))]
        near = sum(p.near_tie for p in picks)
        eps = np.array([p.eps for p in picks])
        rel = np.array([p.gap for p in picks]) / np.abs([lg[i][p.winner] / np.float32(T) for i, p in enumerate(picks)])
        print(f"T={T}: {near} near-ties of {len(lg)}, eps 2^{np.log2(eps.min()):.1f}..2^{np.log2(eps.max()):.1f}, "
              f"relative gap < 2^-16: {(rel < 2.0 ** -16).sum()}, < 2^-14: {(rel < 2.0 ** -14).sum()}")
        assert near <= S.CAP * len(lg) / 5, near   # far inside: a fifth of the cap
        assert 2.0 ** -18 < eps.min() and eps.max() < 2.0 ** -10


def _caught(mutant, lg, T, seed, P, lo, hi):
    """Steps at which the mutant's token leaves the acceptance rule of the true reference."""
    n = 0
    for i in range(len(lg)):
        step = P + i
        mstep = i if mutant == "step_from_first" else step
        tok = S.sample(lg[i], T, seed, mstep, lo, hi, mutant=None if mutant == "step_from_first" else mutant).winner
        n += not S.accepted(tok, S.sample(lg[i], T, seed, step, lo, hi))
    return n


def test_mutants_leave_the_rule():
    n = 24
    lg, tied = _logits(n, seed=31), _logits(n, seed=32, tie=True)
    sp = S.SPEECH
    inside = [w for w in S.tie_windows() if w[1] - w[0] > 1]
    narrow = S.narrow_windows(N_VOCAB)
    cases = {
        "step0": [(lg, 0.8, 42, 4, *sp)],
        "step_from_first": [(lg, 0.8, 42, 4, *sp), (lg, 0.8, 679, 139, *sp)],
        "id_rel_lo": [(lg, 0.8, 42, 4, *sp)],
        "no_seed_hi": [(lg, 0.8, (1 << 40) + 679, 4, *sp)],
        "ties_highest": [(tied, 0.0, 42, 4, lo, hi) for lo, hi in inside],
        "hi_inclusive": [(lg, T, 42, 4, lo, hi) for T in (0.0, 0.8) for lo, hi in narrow if hi < N_VOCAB],
        "mul_T": [(lg, 0.05, 42, 4, *sp), (lg, 5.0, 42, 4, *sp)],
        "noise_at_T0": [(tied, 0.0, 42, 4, lo, hi) for lo, hi in inside],
    }
    assert set(cases) == set(S.MUTANTS)
    caught = {m: [_caught(m, *c) for c in cs] for m, cs in cases.items()}
    print(caught)
    # every listed case sees its mutant, except hi_inclusive, which needs the id past the window
    # to win: it must be seen at some window of every temperature
    for m, c in caught.items():
        if m == "hi_inclusive":
            half = len(c) // 2
            assert sum(c[:half]) > 0 and sum(c[half:]) > 0, (m, c)
        else:
            assert all(x > 0 for x in c), (m, c)
    # a prompt of one token cannot see step_from_first (P = 0): the GPU test has longer ones
    assert _caught("step_from_first", lg, 0.8, 42, 0, *sp) == 0


def test_headline_run_largest_draws():
    """bench.py's default run (one warmup utterance with seed 42, three timed ones, 700 tokens each
    over the speech window, the real prompt): seed 42 meets no draw h >> 40 == 2^24 - 1, the first
    and the last timed utterance meet one each (id 12922 at token 521, id 6454 at token 166). Only
    there can the clamp in gumbel() change the headline's tokens. (It does not: the clamped noise,
    16.64, is still the largest possible, and at T 0.8 that id wins either way; the dumped tokens
    and PCM of the builds before and after the clamp are equal, token 166 being 6454 in both.)"""
    import bench
    P = len(bench.prompt_tokens(bench.PROMPT)) - 1
    seeds = [bench.utterance_seed(0, 0)] + [bench.utterance_seed(0, 1000 + s) for s in range(3)]
    assert seeds[0] == 42 and P == 67
    ids = np.arange(*S.SPEECH)
    hits = []
    for seed in seeds:
        for step in range(P, P + 700):
            hit = ids[S.draw(seed, step, ids) == (1 << 24) - 1]
            hits += [(seed, step - P, int(i)) for i in hit]
    assert hits == [(seeds[1], 521, 12922), (seeds[3], 166, 6454)], hits
