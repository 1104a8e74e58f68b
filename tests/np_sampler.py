"""Independent numpy reference of the on-device sampler (csrc/hip/llm_device.h gumbel(),
sample_token(); the partial producers k_lm_head, k_bt_lm_head, k_bt_gumbel; oracle/llm_ref.c
mo_gumbel / mo_sample), and the acceptance rule the sampler tests share.

The sampler: token = argmax over ids in [lo, hi) of  v / T + g(seed, step, id)  for T > 0, of v
alone for T <= 0; the largest value wins, the lowest id on an exact tie; an empty window gives lo;
a forced id >= 0 overrides. g is counter-based Gumbel noise:

    h = mix64(seed ^ mix64(step << 32 | id))            exact uint64 arithmetic
    d = h >> 40                                          24 bits
    u = min(((float)d + 0.5f) * 2^-24, 1 - 2^-24)        f32 operations, as the kernel does them
    g = -log(-log(u))

(float)d + 0.5f rounds to 2^24 for d = 2^24 - 1 (a tie, to even), which without the min gives
u = 1, -log(u) = -0 and g = +inf; the min changes that one value of d only.

Here u is computed with the kernel's f32 operations (they are exactly rounded IEEE operations,
the same on every machine); the perturbed value v / T + g is then evaluated in float64 from that
f32 u, the f32 v and the f32 T.

Near-ties
---------
The kernel evaluates t = v / T + g in f32 with the device's logf, so where the float64 values of
the top two ids are closer than the kernel's rounding, either may win. err() bounds the kernel's
error on one perturbed value from its operations:

  inner logf      L = -logf(u): K_LOG ulp, a relative error <= K_LOG * 2^-23 of L. log(L (1 + r))
                  = log L + r to first order: it enters g as the ABSOLUTE error K_LOG * 2^-23.
  outer logf      g = -logf(L): K_LOG ulp of g, K_LOG * ulp32(g).
  divide          q = v / T, correctly rounded (the HIP build has no fast-math flag, and hipcc
                  rounds f32 division correctly by default): ulp32(q) / 2.
  add             t = q + g: ulp32(t) / 2.
  negations       exact.

  err(q, g) = K_LOG * (2^-23 + ulp32(g)) + ulp32(q) / 2 + ulp32(q + g) / 2
  eps       = MARGIN * (err(winner) + err(runner-up)),  MARGIN = 4

K_LOG: the ROCm install maps logf to the compiler's log expansion (__clang_hip_math.h: logf ->
__builtin_logf) and carries no accuracy table of its own; the device library is the one OpenCL
runs on, whose full profile allows log 3 ulp, and HIP's published math tables list logf tighter
than that. K_LOG = 3 is the larger of the two. The factor 4 covers the first-order step above
(the inner log's relative error turned into an absolute one) and the oracle's glibc logf, which
is compared under the same rule. For the winner of a 12 800-id window at T = 0.8 (q + g about
10, g in [8, 16)) eps is 4 * 2 * (3 * (2^-23 + 2^-20) + 2^-21 + 2^-21) = 2^-15.2 absolute, a
relative 2^-18.5; at T <= 0 nothing is computed and eps is 0.

A step is a near-tie when the float64 gap of its top two is below eps and the two are not
identical inputs (same f32 q and same u, which tie exactly in the kernel too: the lowest id wins
in both). At a near-tie either of the top two ids is accepted; everywhere else the id must be
equal. CAP: near-ties may be at most 1 % of the compared steps of a case.
"""
from collections import namedtuple

import numpy as np

K_LOG = 3.0
MARGIN = 4.0
CAP = 0.01
U_MAX = np.nextafter(np.float32(1.0), np.float32(0.0))  # 1 - 2^-24
F32_MAX = float(np.finfo(np.float32).max)
# |x| at and above which rounding to f32 overflows (halfway between F32_MAX and 2^128)
F32_OVERFLOW = F32_MAX + 2.0 ** 103

Pick = namedtuple("Pick", "winner runner_up gap eps near_tie")


def mix64(x):
    """splitmix64 finalizer on uint64 arrays (wrapping arithmetic)."""
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def draw(seed: int, step: int, ids) -> np.ndarray:
    """The 24-bit draw h >> 40 of (seed, step, id), uint64 array. step and id enter as uint32."""
    ids = np.asarray(ids, np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ctr = (np.uint64((int(step) & 0xFFFFFFFF) << 32)) | ids
    h = mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ mix64(ctr))
    return h >> np.uint64(40)


def u_of_draw(d, clamp: bool = True) -> np.ndarray:
    """u in f32 operations from the 24-bit draw; clamp=False is the formula before the fix."""
    u = (np.asarray(d).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.minimum(u, U_MAX) if clamp else u


def noise_of_u(u) -> np.ndarray:
    """-log(-log(u)) in float64 from the f32 u."""
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(np.asarray(u, np.float32).astype(np.float64)))


def noise(seed: int, step: int, ids) -> np.ndarray:
    return noise_of_u(u_of_draw(draw(seed, step, ids)))


def ulp32(x) -> np.ndarray:
    """Spacing of f32 at |x| (float64 in, float64 out); inf -> inf."""
    a = np.abs(np.asarray(x, np.float64))
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.minimum(a, F32_MAX).astype(np.float32)
        s = np.spacing(f).astype(np.float64)
    return np.where(np.isfinite(a), s, np.inf)


def err(q, g) -> np.ndarray:
    """Bound of the kernel's f32 error on one perturbed value q + g (see the module docstring)."""
    return K_LOG * (2.0 ** -23 + ulp32(g)) + 0.5 * ulp32(q) + 0.5 * ulp32(np.asarray(q) + np.asarray(g))


def window(allow, n_vocab: int):
    """[lo, hi) of an (allow_lo, allow_hi) pair as the C-ABI documents it: a negative lo is 0, a
    negative hi or one past n_vocab is n_vocab."""
    lo = 0 if allow[0] < 0 else int(allow[0])
    hi = n_vocab if (allow[1] < 0 or allow[1] > n_vocab) else int(allow[1])
    return lo, hi


def quotient(v, T) -> np.ndarray:
    """v / T in float64 from f32 v and f32 T, with f32's overflow: the kernel's quotient is +-inf
    where the exact one rounds past the largest f32."""
    with np.errstate(over="ignore", divide="ignore"):
        q = np.asarray(v, np.float32).astype(np.float64) / np.float64(np.float32(T))
    return np.where(np.abs(q) >= F32_OVERFLOW, np.copysign(np.inf, q), q)


MUTANTS = ("step0", "step_from_first", "id_rel_lo", "no_seed_hi", "ties_highest", "hi_inclusive", "mul_T",
           "noise_at_T0")


def sample(logits, T: float, seed: int, step: int, lo: int, hi: int, forced=None, mutant=None) -> Pick:
    """(winner, runner_up, gap, eps, near_tie) of one sampling step over ids [lo, hi).

    runner_up is -1 and gap inf where there is no second id. mutant: one of MUTANTS, a defective
    restatement for the teeth in test_sampler_ref.py (step_from_first is the caller's: it passes
    another step); never set by a parity test."""
    assert mutant is None or mutant in MUTANTS, mutant
    if forced is not None and forced >= 0:
        return Pick(int(forced), -1, np.inf, 0.0, False)
    if mutant == "hi_inclusive":
        hi = min(hi + 1, len(logits))
    if hi <= lo:
        return Pick(int(lo), -1, np.inf, 0.0, False)
    if mutant == "step0":
        step = 0
    if mutant == "no_seed_hi":
        seed = int(seed) & 0xFFFFFFFF
    ids = np.arange(lo, hi)
    v = np.asarray(logits, np.float32)[lo:hi]
    noisy = np.float32(T) > 0 or mutant == "noise_at_T0"
    if noisy:
        if np.float32(T) > 0:
            q = quotient(v, T) if mutant != "mul_T" else v.astype(np.float64) * np.float64(np.float32(T))
        else:
            q = v.astype(np.float64)
        u = u_of_draw(draw(seed, step, ids - lo if mutant == "id_rel_lo" else ids))
        g = noise_of_u(u)
        with np.errstate(invalid="ignore"):
            t = q + g
    else:
        q = v.astype(np.float64)
        u = np.zeros(len(ids), np.float32)
        g = np.zeros(len(ids))
        t = q
    assert not np.isnan(t).any(), "NaN perturbed value: outside the sampler's contract"
    # largest value first; among equals the lowest id (the highest for the mutant)
    order = np.lexsort((-ids if mutant == "ties_highest" else ids, -t))
    w = int(order[0])
    if len(ids) == 1:
        return Pick(int(ids[w]), -1, np.inf, 0.0, False)
    r = int(order[1])
    with np.errstate(invalid="ignore"):
        gap = float(t[w] - t[r]) if t[w] != t[r] else 0.0
    if not noisy:
        return Pick(int(ids[w]), int(ids[r]), gap, 0.0, False)
    eps = float(MARGIN * (err(q[w], g[w]) + err(q[r], g[r])))
    same_inputs = q[w] == q[r] and u[w] == u[r]
    # two infinite values (an overflowed quotient) compare equal in the kernel as they do here
    exact = same_inputs or (np.isinf(t[w]) and t[w] == t[r])
    near = bool(gap < eps) and not exact
    return Pick(int(ids[w]), int(ids[r]), gap, eps if np.isfinite(eps) else 0.0, near)


def accepted(tok: int, p: Pick) -> bool:
    """The acceptance rule: the winner, or at a near-tie either of the top two."""
    return tok == p.winner or (p.near_tie and tok == p.runner_up)


def compare(tokens, logits_rows, T, seed, first_step, lo, hi, sample_fn=sample):
    """Tokens of consecutive steps first_step, first_step + 1, ... against the reference on the
    logits each step sampled from: (list of (i, token, Pick) that the rule rejects, near-tie
    count)."""
    bad, near = [], 0
    for i, tok in enumerate(tokens):
        p = sample_fn(logits_rows[i], T, seed, first_step + i, lo, hi)
        near += p.near_tie
        if not accepted(int(tok), p):
            bad.append((i, int(tok), p))
    return bad, near


# ---------------------------------------------------------------- cases shared by the tests
SPEECH = (260, 260 + 12800)      # the synthetic vocabulary's speech ids (SYNTH_SPEECH0, 12 800 codes)
WIDTHS = (1, 2, 3, 63, 64, 65, 129)
SEEDS = (42, 679, (1 << 40) + 679)
PROMPT_LENS = (1, 5, 140)


def narrow_windows(n_vocab: int, rng_seed: int = 5):
    """Windows of every width in WIDTHS at offset 0, at n_vocab - width and at three seeded random
    offsets: (lo, hi) pairs."""
    rng = np.random.default_rng(rng_seed)
    out = []
    for w in WIDTHS:
        offs = [0, n_vocab - w] + [int(o) for o in rng.integers(1, n_vocab - w, 3)]
        out += [(o, o + w) for o in offs]
    return out


def wide_cases(n_vocab: int):
    """(name, T, allow) of the wide-window cases; allow as passed to generate."""
    return [("T0.8 speech", 0.8, SPEECH), ("T5 speech", 5.0, SPEECH), ("T0.05 speech", 0.05, SPEECH),
            ("T0.05 all", 0.05, (-1, -1)), ("T0.8 clipped", 0.8, (0, n_vocab + 1000))]


def prompt(n: int, seed: int = 3):
    """A prompt of n byte tokens (ids < 256)."""
    return [int(t) for t in np.random.default_rng(seed + n).integers(0, 256, n)]


TIE_A, TIE_N = 3000, 700  # the tie file: rows [TIE_A, TIE_A + TIE_N) of the output matrix are one row
BATCH_TOKENS = 24


def tie_windows(rng_seed: int = 6):
    """Windows of every width in WIDTHS inside the tie block: at its start, at its end and at three
    seeded random offsets."""
    rng = np.random.default_rng(rng_seed)
    out = []
    for w in WIDTHS:
        offs = [0, TIE_N - w] + [int(o) for o in rng.integers(1, TIE_N - w, 3)]
        out += [(TIE_A + o, TIE_A + o + w) for o in offs]
    return out


def batch_cases(n_vocab: int):
    """The batched-decode cases: dicts of name, tie (the tie file or the plain one), B, prompts,
    seeds, T, allow. Ragged prompts with a single-token one, per-stream seeds with 679 and a
    seed above 2^32; one wide and two narrow windows, and two windows inside the tie block."""
    lens = (5, 1, 140, 9, 33, 2, 64, 17, 100)
    seeds = (679, (1 << 40) + 679, 42, 2199, 706, 7, (1 << 63) + 1, 1000, 1001)
    kinds = (("T0.8 speech", False, 0.8, SPEECH), ("T0.05 speech", False, 0.05, SPEECH),
             ("T5 clipped", False, 5.0, (0, n_vocab + 1000)), ("T0.8 last 65", False, 0.8, (n_vocab - 65, n_vocab)),
             ("T0 width 3", False, 0.0, (4001, 4004)), ("tie T0", True, 0.0, (TIE_A + 3, TIE_A + 3 + 129)),
             ("tie T0.8", True, 0.8, (TIE_A + TIE_N - 65, TIE_A + TIE_N)))
    out = []
    for B in (3, 9):
        for name, tie, T, allow in kinds:
            out.append(dict(name=f"B{B} {name}", tie=tie, B=B, prompts=[prompt(n, 50 + b) for b, n in enumerate(lens[:B])],
                            seeds=list(seeds[:B]), T=T, allow=allow))
    return out
