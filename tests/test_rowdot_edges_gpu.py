"""GPU: the quantized row dots on hand-built blocks at the integer ceilings (tests/np_rowdot.py:
encoders, weight and activation cases, the exact reference and its bound - the operation count
behind the bound is in that module's docstring).

 * mio_hip_debug_matvec: finite, |y - y_ref| <= bound per row, a zero activation gives exactly 0;
 * mio_hip_debug_matvec_group: the bits of debug_matvec for every su the header documents for the
   shape (k <= 2048: 2, 3, 4, 6; k <= 6144: 3), on the smallest grid >= 2 whose waves own at most
   su units;
 * mio_hip_debug_mmq mode 0: the bits of debug_matvec token by token, the tokens of one call
   being different activation cases with `zero` among them: nt 1, 5, 16 (16 x 16 tiles), 17, 33
   (32 x 32 tiles) and 4200 rows at k = 256 (the tile-walking kernel); mode 1 = mode 0 + residual;
 * the SwiGLU epilogue (debug_matvec_swiglu, debug_matvec_group with an up matrix, debug_mmq mode
   2) with gates placed at about 0, +-1, +-20, +-100, +-1e4: finite, and per element within
   2 (E + 3) u |want| + floor of float64 silu(g) * u on the GPU's own plain g and u. The epilogue
   is silu_f (llm_device.h): x / (1.0f + expf(-x)), built without fast-math, so expf is the
   device library's, whose documented maximum error is E = 1 ulp (HIP math API reference,
   single-precision table: expf, 1 ULP); an ulp is at most 2 u, so the first-order count is
   2 E u (expf; its weight e^-g / (1 + e^-g) <= 1) + u (the add) + u (the correctly rounded
   division) + u (the product) = 5 u <= 2 (E + 3) u = 8 u. floor = 2^-126 (1 + |u|): the product
   or silu(g) itself in the subnormal range. That covers g = -100 and -1e4: 1 + expf(-g)
   overflows to inf for g < -88.72 and the quotient is -0 where silu(g) = g e^g is 3.7e-42 or
   less. For -103 < g < -88.72 silu(g) is a NORMAL float32 (up to 2.6e-37) that this expression,
   which is ggml's own (ggml_silu_f32), still returns as -0: ggml is as wrong there as the
   kernel, and no gate of this file is placed in that range.

Combinations (listed by _combos, no random sample): per type, weight case i at width j meets
activation (i + j) mod 8 with rows[(i + j) mod 4]; activation a at width j meets weight case
(a + 2 j + 3) mod 7 with rows[(a + j + 1) mod 4]; rows = (1, 9, 17, 37). So every weight case
meets every width of every type and every activation meets every width. Types 2 and 6 (run as
Q8_0): k = 576, ceiling and random_bytes, activations ramp and outlier.

No output of these tests is MIO_DEBUG_SENTINEL_F32 (a row no wave wrote), asserted on every call.

Measured worst err / bound on an MI355X (a record, not the threshold):
  debug_matvec     type 8: 0.081   12: 0.18   13: 0.19   14: 0.13   30: 0.17   2: 0.094   6: 0.085
                   (worst cases: random_bytes for the integer types - against the outlier,
                   zero_block and const_neg activations - and random bf16 bits against alternating)
  SwiGLU epilogue  type 8: 0.25    12: 0.22   13: 0.26   14: 0.21   30: 0.26
  every bit comparison (group stream, matmul modes 0 / 1, tile walk, mode 2 = matvec_swiglu) equal.
"""
import numpy as np
import pytest

import miotts_amd as m
import np_rowdot as rd

pytestmark = pytest.mark.gpu

ROWS = (1, 9, 17, 37)
TOKEN_ACTS = ("ramp", "zero", "outlier", "const_neg", "alternating", "one_hot", "zero_block", "const_pos")
MMQ_TYPES = (8, 12, 13, 14)
U = 2.0 ** -24
EXPF_ULP = 1

_W, _X, _REF, _Y = {}, {}, {}, {}


def _combos(qtype):
    if qtype in (2, 6):
        return [(c, a, 576, 9) for c in ("ceiling", "random_bytes") for a in ("ramp", "outlier")]
    ks, out = rd.WIDTHS[qtype], []
    for i, case in enumerate(rd.WEIGHT_CASES):
        for j, k in enumerate(ks):
            out.append((case, rd.ACT_CASES[(i + j) % 8], k, ROWS[(i + j) % 4]))
    for a, act in enumerate(rd.ACT_CASES):
        for j, k in enumerate(ks):
            out.append((rd.WEIGHT_CASES[(a + 2 * j + 3) % 7], act, k, ROWS[(a + j + 1) % 4]))
    return sorted(set(out))


def _weights(qtype, case, k, rows):
    key = (qtype, case, k, rows)
    if key not in _W:
        _W[key] = rd.repacked_case(qtype, case, rows, k) if qtype in (2, 6) else rd.weight_case(qtype, case, rows, k)
    return _W[key]


def _act(qtype, act, k):
    key = (rd.act_blk(qtype if qtype not in (2, 6) else 8), act, k)
    if key not in _X:
        _X[key] = rd.act_case(act, k, key[0])
        _X[key].setflags(write=False)
    return _X[key]


def _reference(qtype, case, act, k, rows):
    """(y_ref, bound) float64 [rows], computed once and shared."""
    key = (qtype, case, act, k, rows)
    if key not in _REF:
        f, _ = _weights(qtype, case, k, rows)
        t = 8 if qtype in (2, 6) else qtype
        y, s_abs, maxw, maxa = rd.reference(t, f, _act(qtype, act, k), k)
        _REF[key] = (y, rd.bound(t, k, s_abs, maxw, maxa))
    return _REF[key]


def _no_sentinel(y):
    assert not (np.ascontiguousarray(y).view(np.uint32) == m.SENTINEL_F32).any(), "a row no wave wrote"
    return y


def _matvec(device, qtype, case, act, k, rows):
    """debug_matvec of the combination, run once and shared by the bit comparisons."""
    key = (qtype, case, act, k, rows)
    if key not in _Y:
        _Y[key] = _no_sentinel(m.debug_matvec(device, qtype, _weights(qtype, case, k, rows)[1], k, _act(qtype, act, k)))
        _Y[key].setflags(write=False)
    return _Y[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _group_grid(rows, k, su, nm):
    """The smallest grid >= 2 on which no wave owns more than su units (the shares of
    launch_debug_matvec_group: wave_range's split over grid workgroups of 8 waves)."""
    npass = rd.n_pass(k)
    for grid in range(2, 65):
        ok = True
        for b in range(grid):
            n = rows * (b + 1) // grid - rows * b // grid
            ok &= all((n * (w + 1) // 8 - n * w // 8) * npass * nm <= su for w in range(8))
        if ok:
            return grid
    raise AssertionError((rows, k, su, nm))


@pytest.mark.parametrize("qtype", rd.TYPES + (2, 6))
def test_matvec_inside_bound(device, qtype):
    bad, worst = [], (0.0, None)
    for case, act, k, rows in _combos(qtype):
        y = _matvec(device, qtype, case, act, k, rows).astype(np.float64)
        want, bound = _reference(qtype, case, act, k, rows)
        err = np.abs(y - want)
        if not np.all(np.isfinite(y)):
            bad.append(("not finite", case, act, k, rows))
        elif np.any(err > bound):
            r = int(np.argmax(err - bound))
            bad.append(("bound", case, act, k, rows, r, float(y[r]), float(want[r]), float(err[r] / bound[r]) if bound[r] else np.inf))
        if act == "zero" and y.any():
            bad.append(("zero activation", case, act, k, rows))
        nz = bound > 0
        if nz.any() and np.all(np.isfinite(y)):
            worst = max(worst, (float((err[nz] / bound[nz]).max()), (case, act, k, rows)), key=lambda t: t[0])
        if (~nz).any():  # nothing to sum: the row is exactly 0
            assert not err[~nz].any(), (case, act, k, rows)
    print(f"type {qtype}: {len(_combos(qtype))} combinations, worst err / bound {worst[0]:.3g} at {worst[1]}")
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("qtype", rd.TYPES)
def test_group_stream_equals_matvec(device, qtype):
    bad, n = [], 0
    for case, act, k, rows in _combos(qtype):
        ref = _bits(_matvec(device, qtype, case, act, k, rows))
        for su in ((2, 3, 4, 6) if k <= 2048 else (3,)):
            got = _no_sentinel(m.debug_matvec_group(device, qtype, _weights(qtype, case, k, rows)[1], None, k,
                                                    _act(qtype, act, k), su, _group_grid(rows, k, su, 1)))
            n += 1
            if not np.array_equal(_bits(got), ref):
                bad.append((case, act, k, rows, su, np.flatnonzero(_bits(got) != ref)[:6].tolist()))
    print(f"type {qtype}: {n} group launches")
    assert not bad, (len(bad), bad[:8])


def _mmq_cases(qtype):
    """(case, k, rows, nt): both tile sizes, every weight case, every width at least once."""
    ks, out = rd.WIDTHS[qtype], []
    for i, nt in enumerate((1, 5, 16, 17, 33)):
        out.append((rd.WEIGHT_CASES[i], ks[i % len(ks)], ROWS[1 + i % 3], nt))
        out.append((rd.WEIGHT_CASES[(i + 5) % 7], ks[(i + 2) % len(ks)], ROWS[1 + (i + 1) % 3], nt))
    return out


def _check_mmq(device, qtype, raw, k, x, refs, tag, bad):
    nt, rows = x.shape[0], raw.shape[0]
    y0 = _no_sentinel(m.debug_mmq(device, qtype, raw, k, x))
    for t in range(nt):
        if not np.array_equal(_bits(y0[t]), _bits(refs[t])):
            bad.append((tag, "mode 0", t, np.flatnonzero(_bits(y0[t]) != _bits(refs[t]))[:6].tolist()))
    r0 = np.random.default_rng(nt * 1000 + rows).standard_normal((nt, rows)).astype(np.float32)
    y1 = m.debug_mmq(device, qtype, raw, k, x, mode=1, y_in=r0)
    for t in range(nt):
        if not np.array_equal(_bits(y1[t]), _bits(refs[t] + r0[t])):
            bad.append((tag, "mode 1", t))


@pytest.mark.parametrize("qtype", MMQ_TYPES)
def test_mmq_equals_matvec(device, qtype):
    bad = []
    for case, k, rows, nt in _mmq_cases(qtype):
        acts = [TOKEN_ACTS[t % 8] for t in range(nt)]
        x = np.stack([_act(qtype, a, k) for a in acts])
        refs = [_matvec(device, qtype, case, a, k, rows) for a in acts]
        _check_mmq(device, qtype, _weights(qtype, case, k, rows)[1], k, x, refs, (case, k, rows, nt), bad)
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("qtype", MMQ_TYPES)
def test_mmq_tile_walk_equals_matvec(device, qtype):
    """4200 rows (more 16-row tiles than the chip has CUs), k = 256: the 40 rows of a case, repeated."""
    bad, k, nt = [], 256, 5
    raw = np.tile(np.concatenate([_weights(qtype, "random_bytes", k, 37)[1][:20], _weights(qtype, "ceiling", k, 37)[1][:20]]),
                  (105, 1))
    x = np.stack([_act(qtype, TOKEN_ACTS[t], k) for t in range(nt)])
    refs = [_no_sentinel(m.debug_matvec(device, qtype, raw, k, x[t])) for t in range(nt)]
    assert all(np.array_equal(_bits(r[:40]), _bits(r[40 * 57:40 * 58])) for r in refs)
    _check_mmq(device, qtype, raw, k, x, refs, ("tile walk", k, 4200, nt), bad)
    assert not bad, (len(bad), bad[:8])


# ------------------------------------------------------------------ the SwiGLU epilogue
GATES = (0.0, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4, 0.3, -5.0, 60.0, -60.0)
SWIGLU_K = {8: (576, 2080), 30: (576, 2080), 12: (256, 2048, 2304), 13: (256, 2048, 2304), 14: (256, 2048, 2304)}


def _swiglu_weights(qtype, k, rows=37):
    """gate rows whose plain product is about GATES[row mod 13] (one d per row, chosen from the
    reference of the same codes with d = 1), and moderate up rows."""
    x = _act(qtype, "outlier", k)
    f, _ = rd.weight_case(qtype, "scales_only", rows, k, seed=1)
    target = np.array([GATES[r % len(GATES)] for r in range(rows)])
    if qtype == 30:
        w = np.random.default_rng(k).standard_normal((rows, k)).astype(np.float32)
        f = {"bits": rd._bf16_bits(w)}
        r0 = rd.reference(30, f, x, k)[0]
        f = {"bits": rd._bf16_bits(rd.values(30, f) * (target / r0)[:, None])}
    else:
        for key in ("d", "dmin"):
            if key in f:
                f[key] = np.ones_like(f[key])
        r0 = rd.reference(qtype, f, x, k)[0]
        for key in ("d", "dmin"):
            if key in f:
                f[key] = ((target / r0)[:, None] * np.ones(f[key].shape)).astype(np.float16)
        assert np.all(np.isfinite(f["d"].astype(np.float64)))
    return rd.encode(qtype, f), rd.weight_case(qtype, "scales_only", rows, k, seed=2)[1], x


def _check_swiglu(y, g, u, tag, bad):
    g64, u64 = g.astype(np.float64), u.astype(np.float64)
    with np.errstate(over="ignore"):
        want = g64 / (1.0 + np.exp(-g64)) * u64
    bound = 2 * (EXPF_ULP + 3) * U * np.abs(want) + 2.0 ** -126 * (1 + np.abs(u64))
    err = np.abs(y.astype(np.float64) - want)
    if not np.all(np.isfinite(y)):
        bad.append((tag, "not finite"))
    elif np.any(err > bound):
        r = int(np.argmax(err / bound))
        bad.append((tag, r, float(g[r]), float(u[r]), float(y[r]), float(want[r]), float(err[r] / bound[r])))
    return float((err / bound).max()) if np.all(np.isfinite(y)) else np.inf


@pytest.mark.parametrize("qtype", rd.TYPES)
def test_swiglu_epilogue_at_large_gates(device, qtype):
    bad, worst = [], 0.0
    for k in SWIGLU_K[qtype]:
        wg, wu, x = _swiglu_weights(qtype, k)
        g = _no_sentinel(m.debug_matvec(device, qtype, wg, k, x))
        u = _no_sentinel(m.debug_matvec(device, qtype, wu, k, x))
        hit = [float(np.abs(g - t).min()) <= 0.05 * abs(t) + 1e-30 for t in GATES]
        assert all(hit), (k, g[:13])  # the gates are where the case wants them
        y = _no_sentinel(m.debug_matvec_swiglu(device, qtype, wg, wu, k, x))
        worst = max(worst, _check_swiglu(y, g, u, ("matvec_swiglu", k), bad))
        for su in ((2, 4, 6) if k <= 2048 else ()):
            got = _no_sentinel(m.debug_matvec_group(device, qtype, wg, wu, k, x, su, _group_grid(37, k, su, 2)))
            if not np.array_equal(_bits(got), _bits(y)):
                bad.append(("group swiglu", k, su))
        if qtype in MMQ_TYPES:
            for nt in (5, 17):
                xs = np.stack([_act(qtype, ("outlier", "zero", "ramp")[t % 3], k) for t in range(nt)])
                g0 = _no_sentinel(m.debug_mmq(device, qtype, wg, k, xs))
                u0 = _no_sentinel(m.debug_mmq(device, qtype, wu, k, xs))
                y2 = _no_sentinel(m.debug_mmq(device, qtype, wg, k, xs, mode=2, up_rows=wu))
                if not np.array_equal(_bits(y2[0]), _bits(y)):
                    bad.append(("mmq mode 2 != matvec_swiglu", k, nt))
                for t in range(nt):
                    worst = max(worst, _check_swiglu(y2[t], g0[t], u0[t], ("mmq mode 2", k, nt, t), bad))
    print(f"type {qtype}: worst err / bound {worst:.3g}")
    assert not bad, (len(bad), bad[:8])
