"""Independent numpy reference of the on-device sampler chain (csrc/hip/llm_sample_chain.hip
k_sample_chain; include/mio_hip.h mio_sampling), and the acceptance rule its tests share. The noise,
ulp32 and the near-tie rule are np_sampler's (imported, not copied).

The chain, per step and stream, over the window W = [lo, hi):

  history    H = the last repeat_last_n tokens this generate SAMPLED (prompt and forced tokens are
             no history).
  penalties  for each id in H and W, c = its occurrences in H:
                 l = l / repeat_penalty if l > 0 else l * repeat_penalty
                 l = l - (c * frequency_penalty + presence_penalty)
             every operation rounded to f32, in this order (done here with numpy f32 scalars, which
             are IEEE operations: the result must equal the kernel's bit for bit).
  order      ids by l' descending, then id ascending; every cut keeps a prefix, the first id stays.
  top-k      the first k ids (k <= 0 or k >= |W|: off). Exact.
  top-p      over the top-k survivors w_i = exp(l'_i - l'_max), Z = sum w; id i stays iff the mass
             of the ids before it is < top_p * Z (>= 1: off; <= 0: one id).
  min-p      id i stays iff l'_i >= l'_max + log(min_p) (<= 0: off).
  draw       argmax over the kept ids of l' / T + gumbel(seed, step, id) (T <= 0: of l').

Everything after the penalties is evaluated in float64 on the f32 values l'.

What the kernel computes, and the error bound of the cut
--------------------------------------------------------
top-p. The kernel's mass of id i is the INTEGER q_i = floor(expf(d_i) * 2^40), d_i = fl32(l'_i -
l'_max) (d_i = 0 where l'_i == l'_max), summed exactly with integer atomics; the target is
Tq = max(1, floor(double(top_p) * double(Z_q))), and id i stays iff the integer mass before it is
< Tq. Against the exact w_i = exp(l'_i - l'_max):

  subtraction    d_i correctly rounded: |d_i - d| <= ulp32(d) / 2, a RELATIVE error of w of the same
                 size (e^x - 1 = x to first order).
  expf           K_EXP ulp of its result, a relative K_EXP * 2^-23. K_EXP = 3: the bound OpenCL's
                 full profile gives exp, for the device library HIP's expf maps to (np_sampler's
                 reasoning for K_LOG).
  floor          < 2^-40 absolute (also covers a result flushed to zero below 2^-126).
  d_i == 0       expf(0) is exactly 1 (IEEE 754 9.2.1 requires it of a conforming exp; the device
                 library's range reduction leaves 2^0 * 1), and 2^40 is an integer: such a term has
                 NO error. This is what makes an all-equal row exact.

  e_i  = MARGIN * w_i * (K_EXP * 2^-23 + ulp32(d_i) / 2) + 2^-40     (0 where d_i == 0)
  EC_i = sum of e_j over the ids before i;  EZ = sum of all e_j
  ET   = top_p * EZ + 2^-40 + Z * 2^-51  (the target's floor and the double product's rounding),
         or 0 where EZ == 0: then Z_q is an exact integer below 2^53 and the reference evaluates
         Tq with the kernel's own double operations.

  id i (i >= 1) surely stays    iff C_i + EC_i < Tq * 2^-40 - ET
                may stay        iff C_i - EC_i < Tq * 2^-40 + ET

MARGIN (np_sampler's 4) covers the first-order steps. For a 12,800-id N(0, 1) row the relative
uncertainty of the mass comes to about 4 * (3 * 2^-23 + 2^-22) = 2.4e-6.

min-p. The kernel compares l'_i with thr = fl32(l'_max + logf(min_p)):
  E_m = MARGIN * K_LOG * ulp32(log(min_p)) + ulp32(thr) / 2
  id i surely stays iff l'_i >= thr + E_m, may stay iff l'_i >= thr - E_m (min_p > 1: no id passes
  and the first id stays alone).

So the kept count of a top-p / min-p case is known only as a range [m_lo, m_hi] (the minimum of the
cuts' ranges, inside the exact top-k count). A token is accepted iff, for some prefix length m in
that range, it is the winner of the draw over the first m ids, or its runner-up at a near-tie
(np_sampler's rule: eps from np_sampler.err). A step is AMBIGUOUS when the prefixes of the range
have more than one winner; ambiguous steps and near-ties are each capped at np_sampler.CAP of a
case's steps: a condition on the case lists, asserted on the CPU (test_sampler_chain_ref.py).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import np_sampler as S

K_EXP = 3.0

Params = namedtuple("Params", "top_k top_p min_p repeat_penalty frequency_penalty presence_penalty repeat_last_n")
NEUTRAL = Params(0, 1.0, 0.0, 1.0, 0.0, 0.0, 64)


def params(**kw) -> Params:
    return NEUTRAL._replace(**kw)


MUTANTS = ("p_cross_excluded", "topk_ties_highest", "probs_at_T", "prompt_as_history", "penalty_swap", "no_count",
           "long_history", "minp_vs_sum")

Chain = namedtuple("Chain", "row order m_lo m_hi winners ambiguous t q g u")


def penalise(logits, history, P: Params, lo: int, hi: int, mutant=None) -> np.ndarray:
    """The row after the penalties (a copy, f32); ids outside the history keep their bits."""
    row = np.array(logits, np.float32, copy=True)
    n = int(P.repeat_last_n)
    H = [int(t) for t in history]
    if mutant != "long_history":
        H = H[max(0, len(H) - n):]
    if n <= 0:
        H = []
    rp, fp, pp = np.float32(P.repeat_penalty), np.float32(P.frequency_penalty), np.float32(P.presence_penalty)
    for tok in sorted(set(H)):
        if not lo <= tok < hi:
            continue
        c = np.float32(1 if mutant == "no_count" else H.count(tok))
        l = row[tok]
        with np.errstate(over="ignore", invalid="ignore"):
            if mutant == "penalty_swap":
                l = np.float32(l / rp)
            else:
                l = np.float32(l / rp) if l > 0 else np.float32(l * rp)
            l = np.float32(l - np.float32(np.float32(c * fp) + pp))
        row[tok] = l
    return row


def _top_p_range(s, w, d, p, mutant):
    """[m_lo, m_hi] of the top-p cut over the sorted survivors (values s, masses w, exponents d)."""
    n = len(s)
    p32 = np.float64(max(np.float32(p), np.float32(0)))
    rel = K_EXP * 2.0 ** -23 + 0.5 * S.ulp32(np.where(np.isfinite(d), d, 0.0))
    e = np.where(d == 0, 0.0, S.MARGIN * w * rel + 2.0 ** -40)  # d = -inf: w = 0, the floor's term alone
    C = np.concatenate([[0.0], np.cumsum(w)[:-1]])
    EC = np.concatenate([[0.0], np.cumsum(e)[:-1]])
    Z, EZ = float(np.sum(w)), float(np.sum(e))
    Tq = max(1.0, np.floor(p32 * np.float64(Z * 2.0 ** 40))) * 2.0 ** -40
    ET = 0.0 if EZ == 0 else float(p32 * EZ + 2.0 ** -40 + Z * 2.0 ** -51)
    if mutant == "p_cross_excluded":
        C = C + w
    sure = C + EC < Tq - ET
    may = C - EC < Tq + ET
    sure[0] = may[0] = True
    m_lo = n if sure.all() else int(np.argmin(sure))
    m_hi = n if may.all() else int(np.argmin(may))
    return m_lo, m_hi


def _min_p_range(s, w, mp, mutant):
    n = len(s)
    mp32 = np.float32(mp)
    if mutant == "minp_vs_sum":
        keep = w / np.sum(w) >= np.float64(mp32)
        m = max(1, n if keep.all() else int(np.argmin(keep)))
        return m, m
    L = np.log(np.float64(mp32))
    thr = s[0] + L
    if mp32 > 1:
        return 1, 1
    Em = S.MARGIN * S.K_LOG * float(S.ulp32(L)) + 0.5 * float(S.ulp32(thr))
    with np.errstate(invalid="ignore"):
        sure = s >= thr + Em
        may = s >= thr - Em
    sure[0] = may[0] = True
    return (n if sure.all() else int(np.argmin(sure))), (n if may.all() else int(np.argmin(may)))


def chain(logits, history, P: Params, T: float, seed: int, step: int, lo: int, hi: int, prompt=(), mutant=None):
    """The chain on one row: the penalised row, the ids in order, the range of admissible kept counts,
    the winners of those prefixes (winners[0] for the smallest), whether they differ, and the
    perturbed values of the window (t = q + g, float64; u the f32 draw) for the acceptance rule.
    None for an empty window (the token is lo)."""
    assert mutant is None or mutant in MUTANTS, mutant
    if hi <= lo:
        return None
    hist = (list(prompt) + list(history)) if mutant == "prompt_as_history" else list(history)
    row = penalise(logits, hist, P, lo, hi, mutant)
    v = row[lo:hi].astype(np.float64)
    assert not np.isnan(v).any()
    ids = np.arange(lo, hi)
    order = np.lexsort((-ids if mutant == "topk_ties_highest" else ids, -v))
    n = hi - lo
    k = n if (P.top_k <= 0 or P.top_k >= n) else int(P.top_k)
    s = v[order[:k]]
    with np.errstate(invalid="ignore"):
        d = np.where(s == s[0], 0.0, s - s[0])
    Tw = np.float64(np.float32(T)) if (mutant == "probs_at_T" and np.float32(T) > 0) else 1.0
    w = np.exp(d / Tw)
    m_lo = m_hi = k
    if np.float32(P.top_p) < 1:
        a, b = _top_p_range(s, w, d, P.top_p, mutant)
        m_lo, m_hi = min(m_lo, a), min(m_hi, b)
    if np.float32(P.min_p) > 0:
        a, b = _min_p_range(s, w, P.min_p, mutant)
        m_lo, m_hi = min(m_lo, a), min(m_hi, b)
    assert 1 <= m_lo <= m_hi <= k
    # the draw's perturbed values over the whole window
    if np.float32(T) > 0:
        q = S.quotient(row[lo:hi], T)
        u = S.u_of_draw(S.draw(seed, step, ids))
        g = S.noise_of_u(u)
        with np.errstate(invalid="ignore"):
            t = q + g
    else:
        q, u, g = v, np.zeros(n, np.float32), np.zeros(n)
        t = v
    assert not np.isnan(t[order[:m_hi]]).any()
    # winners of the prefixes m_lo .. m_hi: the first prefix's, then every later id that beats the
    # running best (largest value, lowest id among equals)
    first = order[:m_lo]
    b = first[np.lexsort((ids[first], -t[first]))[0]]
    winners = [int(b)]
    rest = order[m_lo:m_hi]
    if len(rest):
        cand = rest[t[rest] >= t[b]]
        for j in cand:
            if t[j] > t[b] or (t[j] == t[b] and ids[j] < ids[b]):
                b = j
                winners.append(int(b))
    return Chain(row, lo + order, m_lo, m_hi, [lo + x for x in winners], len(winners) > 1, t, q, g, u)


Verdict = namedtuple("Verdict", "ok near_tie ambiguous")


def accept(tok: int, c: Chain, lo: int, T: float, kept=None) -> Verdict:
    """The acceptance rule: tok is the winner of the smallest admissible prefix that contains it, or
    its runner-up at a near-tie (np_sampler's eps). Larger prefixes only add competitors.
    kept: the kept count the kernel itself reported (the one-launch entry): the prefix is then that
    one, admissible or the token is rejected, so a draw over another count than the reported one
    does not pass."""
    order = c.order - lo
    pos = np.nonzero(order == tok - lo)[0]
    if len(pos) == 0 or pos[0] >= c.m_hi:
        return Verdict(False, False, c.ambiguous)
    m = max(c.m_lo, int(pos[0]) + 1)
    if kept is not None:
        if not (c.m_lo <= kept <= c.m_hi) or pos[0] >= kept:
            return Verdict(False, False, c.ambiguous)
        m = int(kept)
    pre = order[:m]
    rank = pre[np.lexsort((pre, -c.t[pre]))]
    w = rank[0]
    if w == tok - lo:
        near = False
        if m > 1 and np.float32(T) > 0:
            near = _near(c, w, rank[1])
        return Verdict(True, near, c.ambiguous)
    if m > 1 and rank[1] == tok - lo and np.float32(T) > 0 and _near(c, w, rank[1]):
        return Verdict(True, True, c.ambiguous)
    return Verdict(False, False, c.ambiguous)


def _near(c: Chain, w, r) -> bool:
    gap = float(c.t[w] - c.t[r]) if c.t[w] != c.t[r] else 0.0
    eps = float(S.MARGIN * (S.err(c.q[w], c.g[w]) + S.err(c.q[r], c.g[r])))
    exact = (c.q[w] == c.q[r] and c.u[w] == c.u[r]) or (np.isinf(c.t[w]) and c.t[w] == c.t[r])
    return bool(gap < eps) and not exact


def sample(logits, history, P, T, seed, step, lo, hi, forced=None, prompt=(), mutant=None) -> int:
    """The reference's token (the winner of the smallest admissible prefix)."""
    if forced is not None and forced >= 0:
        return int(forced)
    c = chain(logits, history, P, T, seed, step, lo, hi, prompt, mutant)
    return int(lo) if c is None else c.winners[0]


# ---------------------------------------------------------------- cases shared by the tests
N_VOCAB = 13312  # the tiny presets' vocabulary (260 byte-level and control ids + 12,800 speech + padding)
WIDTHS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 12800)
FAMILIES = ("n1", "n4", "zipf")


def family_row(kind: str, rng, n: int = N_VOCAB) -> np.ndarray:
    if kind == "n1":
        return rng.standard_normal(n).astype(np.float32)
    if kind == "n4":
        return (2.0 * rng.standard_normal(n)).astype(np.float32)
    assert kind == "zipf"
    return (-1.1 * np.log(1.0 + rng.permutation(n))).astype(np.float32)


def windows(n_vocab: int = N_VOCAB, rng_seed: int = 11):
    """Every width in WIDTHS at offset 0, at n_vocab - width and at one seeded offset."""
    rng = np.random.default_rng(rng_seed)
    out = []
    for w in WIDTHS:
        offs = [0, n_vocab - w, int(rng.integers(1, n_vocab - w))]
        out += [(o, o + w) for o in offs]
    return out


def _case(name, row, lo, hi, P, T=0.8, seed=42, step=None, history=(), exact=False):
    history = [int(t) for t in history]
    return dict(name=name, row=row, lo=lo, hi=hi, P=P, T=T, seed=seed, step=len(history) + 5 if step is None else step,
                history=history, exact=exact)


@lru_cache(maxsize=None)
def exact_cases(n_vocab: int = N_VOCAB):
    """Cases whose kept count, cut id and penalised row are exact."""
    rng = np.random.default_rng(21)
    out = []
    for wi, (lo, hi) in enumerate(windows(n_vocab)):
        w = hi - lo
        rows = (("rand", family_row(FAMILIES[wi % 3], rng, n_vocab)), ("equal", np.full(n_vocab, 0.75, np.float32)))
        for rname, row in rows:
            for k in (1, 2, 40, w - 1, w, w + 1, 0):
                T = 0.8 if (k + wi) % 2 else 0.0
                out.append(_case(f"topk{k} {rname} [{lo},{hi})", row, lo, hi, params(top_k=k), T, S.SEEDS[wi % 3],
                                 exact=True))
    eq = np.full(n_vocab, -1.5, np.float32)
    for lo in (0, 1000, n_vocab - 64):
        out.append(_case(f"topp.5 equal64 @{lo}", eq, lo, lo + 64, params(top_p=0.5), exact=True))
        out.append(_case(f"topp.3 equal64 @{lo}", eq, lo, lo + 64, params(top_p=0.3), exact=True))
    out.append(_case("topp.5 equal1025", eq, 7, 7 + 1025, params(top_p=0.5), exact=True))
    out.append(_case("topk100 topp.3 equal", eq, 300, 300 + 1025, params(top_k=100, top_p=0.3), exact=True))
    # -inf entries: a row with -inf runs, and a row that is -inf but for three ids
    row = family_row("n1", rng, n_vocab)
    row[rng.integers(0, n_vocab, 4000)] = -np.inf
    few = np.full(n_vocab, -np.inf, np.float32)
    few[[300, 5000, 13000]] = (1.0, 2.0, 2.0)
    for lo, hi in ((0, n_vocab), (260, 260 + 12800), (4990, 5055)):
        for k in (0, 2, 40, 9000):
            out.append(_case(f"-inf topk{k} [{lo},{hi})", row, lo, hi, params(top_k=k), exact=True))
            out.append(_case(f"few topk{k} [{lo},{hi})", few, lo, hi, params(top_k=k), 0.8, 679, exact=True))
    out.append(_case("all -inf topk3", np.full(n_vocab, -np.inf, np.float32), 10, 500, params(top_k=3), exact=True))
    # histories: repeats, ids outside the window, lengths 0, 1, 64, 256 and longer than repeat_last_n
    lo, hi = 260, 260 + 12800
    for hl in (0, 1, 11, 64, 256, 300):
        for last_n in (64, 256, 16, 0):
            hist = rng.integers(lo, lo + 40, hl).tolist()  # 40 ids: repeats from length 64 on
            hist[::7] = rng.integers(0, lo, len(hist[::7])).tolist()  # ids below the window
            row = family_row("n4", rng, n_vocab)
            P = params(repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1, repeat_last_n=last_n, top_k=40)
            out.append(_case(f"hist{hl} last{last_n}", row, lo, hi, P, 0.8, S.SEEDS[hl % 3], history=hist, exact=True))
    hist = [5, 5, 5, 300, 300, 301, 13311, 13311, 0]
    row = family_row("n1", rng, n_vocab)
    out.append(_case("penalties whole vocab", row, 0, n_vocab, params(repeat_penalty=0.7, frequency_penalty=-0.3,
                                                                      presence_penalty=1.5, top_k=5), 0.0, history=hist,
                     exact=True))
    out.append(_case("penalties alone", row, 0, n_vocab, params(repeat_penalty=1.1), 0.8, history=hist, exact=True))
    return out


@lru_cache(maxsize=None)
def ranged_cases(n_vocab: int = N_VOCAB):
    """top-p, min-p and all knobs together on the three row families: the kept count in a range."""
    rng = np.random.default_rng(22)
    out = []
    wins = windows(n_vocab)
    for fi, fam in enumerate(FAMILIES):
        for wi, (lo, hi) in enumerate(wins):
            row = family_row(fam, rng, n_vocab)
            seed = S.SEEDS[(wi + fi) % 3]
            p = (1e-6, 0.5, 0.9, 0.999999)[(wi + fi) % 4]
            mp = (0.05, 0.5, 1.0)[(wi + fi) % 3]
            out.append(_case(f"{fam} topp{p} [{lo},{hi})", row, lo, hi, params(top_p=p), 0.8, seed))
            out.append(_case(f"{fam} minp{mp} [{lo},{hi})", row, lo, hi, params(min_p=mp), 0.8, seed))
        for lo, hi in ((260, 260 + 12800), (0, n_vocab), (3000, 4025)):
            row = family_row(fam, rng, n_vocab)
            for p in (1e-6, 0.5, 0.9, 0.999999):
                out.append(_case(f"{fam} topp{p} wide [{lo},{hi})", row, lo, hi, params(top_p=p), 0.8, 679))
            for mp in (0.05, 0.5, 1.0):
                out.append(_case(f"{fam} minp{mp} wide [{lo},{hi})", row, lo, hi, params(min_p=mp), 0.8, 679))
            hist = rng.integers(lo, hi, 80).tolist() + list(lo + np.argsort(-row[lo:hi])[:6]) * 2
            P = params(top_k=50, top_p=0.9, min_p=0.05, repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1,
                       repeat_last_n=64)
            for T in (0.8, 0.0):
                out.append(_case(f"{fam} all T{T} [{lo},{hi})", row, lo, hi, P, T, (1 << 40) + 679, history=hist))
    return out


@lru_cache(maxsize=None)
def neutral_cases(n_vocab: int = N_VOCAB):
    rng = np.random.default_rng(23)
    out = []
    for wi, (lo, hi) in enumerate(windows(n_vocab)):
        row = family_row(FAMILIES[wi % 3], rng, n_vocab)
        out.append(_case(f"neutral [{lo},{hi})", row, lo, hi, NEUTRAL, (0.8, 0.0, 5.0)[wi % 3], S.SEEDS[wi % 3],
                         history=[lo, lo, hi - 1]))
    return out


# The wide model: a vocabulary past the kernel's register-resident window limit (13 * 1024 ids),
# where every pass re-reads the row from memory (its other body). Preset 2, the 0.1B shape.
WIDE_PRESET = 2
WIDE_VOCAB = 61952
REG_LIMIT = 13 * 1024
# just past the limit; wave segments that are no multiple of 256 ids (the body's load stride) nor
# of 64; a segment that is a multiple of 256; the whole vocabulary
WIDE_WIDTHS = (REG_LIMIT + 1, 20001, 16 * 1280, 40007, WIDE_VOCAB)


def wide_windows(n_vocab: int = WIDE_VOCAB, rng_seed: int = 12):
    rng = np.random.default_rng(rng_seed)
    out = []
    for w in WIDE_WIDTHS:
        offs = sorted({0, n_vocab - w, int(rng.integers(0, n_vocab - w + 1))})
        out += [(o, o + w) for o in offs]
    return out


@lru_cache(maxsize=None)
def wide_exact_cases(n_vocab: int = WIDE_VOCAB):
    """The exact kinds of exact_cases on windows wider than REG_LIMIT."""
    rng = np.random.default_rng(31)
    out = []
    eq = np.full(n_vocab, 0.75, np.float32)
    for wi, (lo, hi) in enumerate(wide_windows(n_vocab)):
        w = hi - lo
        row = family_row(FAMILIES[wi % 3], rng, n_vocab)
        for k in (1, 40, w - 1, w + 1):
            out.append(_case(f"wide topk{k} rand [{lo},{hi})", row, lo, hi, params(top_k=k), (0.8, 0.0)[(k + wi) % 2],
                             S.SEEDS[wi % 3], exact=True))
        for k in (2, REG_LIMIT + 5, w - 1):  # a cut inside a run of equals: the lowest k ids
            out.append(_case(f"wide topk{k} equal [{lo},{hi})", eq, lo, hi, params(top_k=k), 0.8, S.SEEDS[wi % 3],
                             exact=True))
        out.append(_case(f"wide topp.3 equal [{lo},{hi})", eq, lo, hi, params(top_p=0.3), exact=True))
        out.append(_case(f"wide topk15000 topp.5 equal [{lo},{hi})", eq, lo, hi, params(top_k=15000, top_p=0.5),
                         exact=True))
        inf = row.copy()
        inf[rng.integers(0, n_vocab, n_vocab // 3)] = -np.inf
        out.append(_case(f"wide -inf topk9000 [{lo},{hi})", inf, lo, hi, params(top_k=9000), exact=True))
        for hl, last_n in ((11, 16), (300, 256), (64, 64)):
            hist = rng.integers(lo, lo + 40, hl).tolist()
            hist[::7] = rng.integers(hi, n_vocab, len(hist[::7])).tolist() if hi < n_vocab else hist[::7]
            P = params(repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1, repeat_last_n=last_n, top_k=40)
            out.append(_case(f"wide hist{hl} last{last_n} [{lo},{hi})", row, lo, hi, P, 0.8, S.SEEDS[hl % 3],
                             history=hist, exact=True))
    return out


@lru_cache(maxsize=None)
def wide_ranged_cases(n_vocab: int = WIDE_VOCAB):
    rng = np.random.default_rng(32)
    out = []
    for wi, (lo, hi) in enumerate(wide_windows(n_vocab)):
        fam = FAMILIES[wi % 3]
        row = family_row(fam, rng, n_vocab)
        p = (1e-6, 0.5, 0.9, 0.999999)[wi % 4]
        mp = (0.05, 0.5, 1.0)[wi % 3]
        out.append(_case(f"wide {fam} topp{p} [{lo},{hi})", row, lo, hi, params(top_p=p), 0.8, S.SEEDS[wi % 3]))
        out.append(_case(f"wide {fam} minp{mp} [{lo},{hi})", row, lo, hi, params(min_p=mp), 0.8, S.SEEDS[wi % 3]))
        hist = rng.integers(lo, hi, 80).tolist() + list(lo + np.argsort(-row[lo:hi])[:6]) * 2
        P = params(top_k=50, top_p=0.9, min_p=0.05, repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1,
                   repeat_last_n=64)
        out.append(_case(f"wide {fam} all [{lo},{hi})", row, lo, hi, P, (0.8, 0.0)[wi % 2], (1 << 40) + 679,
                         history=hist))
    return out


@lru_cache(maxsize=None)
def wide_neutral_cases(n_vocab: int = WIDE_VOCAB):
    rng = np.random.default_rng(33)
    return [_case(f"wide neutral [{lo},{hi})", family_row(FAMILIES[wi % 3], rng, n_vocab), lo, hi, NEUTRAL,
                  (0.8, 0.0, 5.0)[wi % 3], S.SEEDS[wi % 3], history=[lo, lo, hi - 1])
            for wi, (lo, hi) in enumerate(wide_windows(n_vocab))]


def run_case(c, mutant=None, prompt=()):
    return chain(c["row"], c["history"], c["P"], c["T"], c["seed"], c["step"], c["lo"], c["hi"], prompt, mutant)


# end to end: the replay scheme of test_sampler_gpu.py with the chain on
E2E_TOKENS = 48
E2E_CONFIGS = (("topk40", params(top_k=40)), ("topp.9", params(top_p=0.9)),
               ("minp+rep", params(min_p=0.05, repeat_penalty=1.3, repeat_last_n=16, frequency_penalty=0.2)),
               ("all", params(top_k=40, top_p=0.9, min_p=0.05, repeat_penalty=1.3, repeat_last_n=16,
                              frequency_penalty=0.2, presence_penalty=0.1)))
E2E_PROMPT_LENS = (5, 140)
E2E_TEMPS = (0.8, 0.0)


# The narrow end-to-end case: 65 ids and a history of 16, so sampled ids do come back, and a prompt
# made of ids of the window itself, so that a chain that took the prompt for history would draw
# other tokens from the first step on.
NARROW = dict(allow=(1260, 1325), P=params(repeat_penalty=1.5, frequency_penalty=0.3, presence_penalty=1.0,
                                          repeat_last_n=16), T=0.8, seed=679, n_prompt=24)


def narrow_prompt(seed: int = 9):
    lo, hi = NARROW["allow"]
    return [int(t) for t in np.random.default_rng(seed).integers(lo, hi, NARROW["n_prompt"])]


def compare_run(tokens, rows, P: Params, T, seed, first_step, lo, hi, prompt=(), mutant=None):
    """Tokens of consecutive steps against the reference on the logits each step sampled from, with the
    run's own earlier tokens as history: (rejected (i, token) list, near-ties, ambiguous steps)."""
    bad, near, amb = [], 0, 0
    for i, tok in enumerate(tokens):
        c = chain(rows[i], [int(t) for t in tokens[:i]], P, T, seed, first_step + i, lo, hi, prompt, mutant)
        v = accept(int(tok), c, lo, T)
        near += v.near_tie
        amb += v.ambiguous
        if not v.ok:
            bad.append((i, int(tok), c.winners))
    return bad, near, amb
