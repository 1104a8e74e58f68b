"""GPU parity of the MioCodec kernels one launch at a time (csrc/hip/codec_kernels.hip through
the mio_hip_debug_codec_* entry points of libmiotts_test.so) against plain float64 numpy.

The stage tests of test_codec_gpu.py hold chains of 10-30 launches of two weight files to
1e-3; here every kernel is held on its own to a bound derived from its arithmetic, at the
shapes the loader accepts but the two presets never reach (K-group counts 1 and 2, odd and
even stage counts, K tails, edge tiles, every row-norm width, GroupNorm with more than 32
groups or a partial 64-channel slice, windows below 65, conv taps 1 and 5, ...).

How a bound is built. u = 2^-24 is the unit roundoff of f32. A quantity is carried as
(value in float64, bound on |device value - value|); `_Q` below propagates the bound through
each f32 operation to first order plus the cross terms (sum: e_a + e_b; product:
|a| e_b + |b| e_a + e_a e_b; quotient, square root and the transcendental functions by their
derivatives) and adds u (|value| + bound) for the operation's own rounding. _TINY = 1e-30 is
added once per operation for results that leave the normal f32 range (silu's tail: expf
overflows where the float64 value is below 1e-36).

  * a dot product of n terms computed by any order of correctly rounded f32 fma and adds is
    within (n + 8) u sum_k |a_k b_k| of the exact one (the MFMA chains, the K-group adds, the
    lane trees); the ROCm documentation states no truncation of the MFMA's internal adds,
    so the constant is 2^-24, not 2^-23;
  * division and sqrtf are correctly rounded (hipcc's default,
    -fhip-fp32-correctly-rounded-divide-sqrt), one u each;
  * the ROCm installation documents no error bound for expf, sinf and cosf, so their allowance was
    measured (test_epilogue_function_allowance, on accumulators that are exact, over the
    arguments these tests produce). Largest deviation from float64 on the MI355X, in units of
    2^-23 (relative for expf, i.e. ulps; absolute for sinf and cosf, |f| <= 1): expf 0.544,
    cosf 0.435, sinf 0.443. The allowances are twice that rounded up to whole units:
    _E_EXP = 2, _E_COS = 1, _E_SIN = 1. The test asserts the deviation stays inside them.

Every element of every output is compared; every test asserts that the guard zones around the
output are intact and that no sentinel is left where the contract says a value is written.
The teeth checks run the same comparison against a deliberately wrong reference and require it
to fail."""
import os
import subprocess
import sys

import numpy as np
import pytest

import miotts_amd as m

pytestmark = pytest.mark.gpu

_U = 2.0 ** -24
_TINY = 1e-30
_E_EXP, _E_SIN, _E_COS = 2, 1, 1   # units of 2^-23: relative (expf), absolute (sinf, cosf)
_SENT32 = np.uint32(m.SENTINEL_F32)
_SENT16 = np.uint16(m.SENTINEL_F16)


class _Q:
    """value (float64) and a bound on |device f32 value - value| (see the module docstring)."""

    def __init__(self, val, err=0.0):
        self.val = np.asarray(val, np.float64)
        self.err = np.broadcast_to(np.asarray(err, np.float64), self.val.shape)

    @staticmethod
    def _rnd(val, err):
        return _Q(val, err + _U * (np.abs(val) + err) + _TINY)

    def __add__(self, o):
        o = _q(o)
        return _Q._rnd(self.val + o.val, self.err + o.err)

    def __sub__(self, o):
        o = _q(o)
        return _Q._rnd(self.val - o.val, self.err + o.err)

    def __mul__(self, o):
        o = _q(o)
        return _Q._rnd(self.val * o.val, np.abs(self.val) * o.err + np.abs(o.val) * self.err + self.err * o.err)

    def __truediv__(self, o):
        o = _q(o)
        den = np.abs(o.val) - o.err
        assert np.all(den > 0)
        val = self.val / o.val
        return _Q._rnd(val, (self.err + np.abs(val) * o.err) / den)

    def neg(self):
        return _Q(-self.val, self.err)

    def sqrt(self):
        lo = np.maximum(self.val - self.err, 1e-300)
        return _Q._rnd(np.sqrt(self.val), self.err / (2.0 * np.sqrt(lo)))

    def exp(self):
        with np.errstate(all="ignore"):
            v = np.exp(self.val)
            g = np.expm1(self.err)
            return _Q(v, v * g + _E_EXP * 2.0 ** -23 * v * (1.0 + g) + _TINY)

    def sin(self):
        return _Q(np.sin(self.val), np.minimum(self.err, 2.0) + _E_SIN * 2.0 ** -23)

    def cos(self):
        return _Q(np.cos(self.val), np.minimum(self.err, 2.0) + _E_COS * 2.0 ** -23)

    def f32(self):
        """the value after a conversion to f32 (a double result cast to float)"""
        return _Q._rnd(self.val, self.err)


def _q(x):
    return x if isinstance(x, _Q) else _Q(x)


def _mean_f32(mu64):
    """(float)(double sum / n): the double sum is exact to ~2^-50, so the kernel's f32 mean is
    the f32 rounding of the float64 mean (it could round the other way only with the float64
    mean within 2^-50 of a rounding boundary; that would show as failures, not pass wrongly)."""
    return _Q(np.asarray(mu64, np.float64).astype(np.float32).astype(np.float64), 2.0 ** -45 * np.abs(mu64))


def _silu(y):
    """silu_f: x / (1.0f + expf(-x))"""
    return y / (_Q(1.0) + y.neg().exp())


def _snake(v, a, b):
    """snake_f: v + sinf(v * a)^2 / b"""
    s = (v * a).sin()
    return v + (s * s) / b


def _dot(a, b, n_terms):
    """sum_k a[.., k] b[.., k] of exact f32 inputs by any order of f32 fma / adds."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return _Q(a @ b.T, (n_terms + 8) * _U * (np.abs(a) @ np.abs(b).T))


def _check(got, want: _Q, what, guards_ok=True):
    got = np.asarray(got)
    assert guards_ok, f"{what}: a guard zone was overwritten"
    assert got.shape == want.val.shape, (what, got.shape, want.val.shape)
    assert not np.any(got.view(np.uint32) == _SENT32), f"{what}: {int(np.sum(got.view(np.uint32) == _SENT32))} elements unwritten"
    d = np.abs(got.astype(np.float64) - want.val)
    bad = ~(d <= want.err)
    if np.any(bad):
        i = np.unravel_index(np.argmax(np.where(bad, d / (want.err + 1e-300), 0)), d.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {d.size} elements outside the bound; worst at {i}: "
                             f"got {got[i]!r} want {want.val[i]!r} |diff| {d[i]:.3g} bound {want.err[i]:.3g}")


def _fails(got, want: _Q) -> bool:
    """teeth: does the comparison reject this (wrong) reference?"""
    got = np.asarray(got)
    if got.shape != want.val.shape:
        return True
    return bool(np.any(~(np.abs(got.astype(np.float64) - want.val) <= want.err)))


def _assert_tight(want: _Q, rms=1e-5):
    """A derived bound must be at least 100x tighter than the stage bar of test_codec_gpu.py
    (1e-3 relative RMS, 5e-3 of the largest value) at the tested size."""
    assert np.sqrt(np.mean(want.err ** 2)) <= rms * np.sqrt(np.mean(want.val ** 2))
    assert np.max(want.err) <= 5e-5 * np.max(np.abs(want.val))


def _seed(*key):
    # hash() of a str changes per process: spell the key out as integers
    out = []
    for k in key:
        if isinstance(k, str):
            out.extend(ord(ch) for ch in k)
        else:
            out.append(int(k) & 0x7FFFFFFF)
    return np.random.default_rng(out)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------ GEMM
def _awin(A, M, K, a_row_off, f16=False):
    """The tap window: element (m, k) = A.flat[(m + a_row_off) * a_seg + k] where that index is
    a row of [0, a_rows), else zero."""
    a_rows, a_seg = A.shape
    idx = (np.arange(M)[:, None] + a_row_off) * a_seg + np.arange(K)[None, :]
    ok = (idx >= 0) & (idx < a_rows * a_seg)
    src = A.astype(np.float16).astype(np.float64) if f16 else A.astype(np.float64)
    return np.where(ok, src.reshape(-1)[np.clip(idx, 0, a_rows * a_seg - 1)], 0.0)


def _gemm_acc(A, B, M, a_row_off=0, f16=False, drop=0):
    K = B.shape[1]
    W = _awin(A, M, K, a_row_off, f16)
    if drop:
        return _dot(W[:, :K - drop], B[:, :K - drop], K)
    return _dot(W, B, K)


def _epi_ref(epi, acc: _Q, C0, p):
    """The epilogue on the accumulators acc [M][N]; returns the expected C as a _Q of C0's shape
    plus the mask of elements the contract writes."""
    M, N = acc.val.shape
    val = C0.astype(np.float64).copy()
    err = np.zeros_like(val)
    wr = np.zeros(val.shape, bool)

    def put(rows, cols, q):
        val[rows, cols], err[rows, cols], wr[rows, cols] = q.val, q.err, True

    bias = p.get("bias")
    if epi == m.EPI_STORE:
        put(slice(0, M), slice(0, N), acc + _Q(bias) if bias is not None else acc)
    elif epi == m.EPI_RESID:
        v = acc + _Q(bias) if bias is not None else acc
        put(slice(0, M), slice(0, N), _Q(C0[:M, :N]) + v)
    elif epi == m.EPI_GATED:
        put(slice(0, M), slice(0, N), _Q(C0[:M, :N]) + acc * _Q(p["aux"]))
    elif epi == m.EPI_SNAKE:
        put(slice(0, M), slice(0, N), _snake(acc + _Q(bias), _Q(p["aux"]), _Q(p["aux2"])))
    elif epi in (m.EPI_SWIGLU, m.EPI_HEAD):
        blk = np.arange(N // 32)[:, None] * 32 + np.arange(16)[None, :]
        lo, hi = blk.reshape(-1), blk.reshape(-1) + 16  # gate | up, logmag | phase columns
        a = _Q(acc.val[:, lo], acc.err[:, lo])
        b = _Q(acc.val[:, hi], acc.err[:, hi])
        if epi == m.EPI_SWIGLU:
            put(slice(0, M), slice(0, N // 2), _silu(a) * b)
        else:
            nf = p["cout"]
            v = a + _Q(bias[lo])
            ph = b + _Q(bias[hi])
            # mag = clamp(expf(v), 0, 100): the clamp of the interval's ends bounds its error
            e = v.exp()
            mag = np.minimum(e.val, 100.0)
            mag_e = np.maximum(np.minimum(e.val + e.err, 100.0) - mag, mag - np.minimum(np.maximum(e.val - e.err, 0), 100.0))
            magq = _Q(mag, mag_e)
            re, im = magq * ph.cos(), magq * ph.sin()
            put(slice(0, M), slice(0, 2 * nf, 2), _Q(re.val[:, :nf], re.err[:, :nf]))
            put(slice(0, M), slice(1, 2 * nf, 2), _Q(im.val[:, :nf], im.err[:, :nf]))
    else:  # ConvT remap
        f, trim, cout, rows_out = p["f"], p["trim"], p["cout"], p["rows_out"]
        n = np.arange(N)
        rr, co = n // cout, n % cout
        orow = f * np.arange(M)[:, None] + rr[None, :] - trim
        v = acc + _Q(bias[co][None, :])
        if epi == m.EPI_CONVT_SNAKE:
            v = _snake(v, _Q(p["aux"][co][None, :]), _Q(p["aux2"][co][None, :]))
        ok = (orow >= 0) & (orow < rows_out)
        cc = np.broadcast_to(co[None, :], orow.shape)
        assert not wr[orow[ok], cc[ok]].any()
        val[orow[ok], cc[ok]], err[orow[ok], cc[ok]], wr[orow[ok], cc[ok]] = v.val[ok], v.err[ok], True
    return _Q(val, err), wr


def _gemm_case(rng, M, N, K, epi, a_row_off=0, a_rows=None, a_seg=None, f16=0, bias=True, **remap):
    """Random operands of one GEMM and the dict of launch arguments."""
    a_seg = a_seg or K
    a_rows = a_rows or M
    p = dict(remap)
    A = _f32(rng.standard_normal((a_rows, a_seg)))
    B = _f32(rng.standard_normal((N, K)))
    if f16:
        B = B.astype(np.float16).astype(np.float32)  # an F16 GGUF matrix, widened at load
    ncol = p["cout"] if epi in (m.EPI_CONVT, m.EPI_CONVT_SNAKE) else N
    if bias:
        p["bias"] = _f32(rng.standard_normal(ncol))
    if epi == m.EPI_GATED:
        p["aux"] = _f32(rng.standard_normal(ncol))
    if epi in (m.EPI_SNAKE, m.EPI_CONVT_SNAKE):
        p["aux"] = _f32(np.exp(0.5 * rng.standard_normal(ncol)))
        p["aux2"] = _f32(np.exp(0.5 * rng.standard_normal(ncol)))
    if epi in (m.EPI_CONVT, m.EPI_CONVT_SNAKE):
        shape = (p["rows_out"] + 3, p["cout"])  # three spare rows past rows_out: never written
    elif epi == m.EPI_SWIGLU:
        shape = (M, N // 2)
    elif epi == m.EPI_HEAD:
        shape = (M, 2 * p["cout"])
    else:
        shape = (M, N)
    if epi in (m.EPI_RESID, m.EPI_GATED):
        C0 = _f32(rng.standard_normal(shape))
    else:
        C0 = m.sentinel_f32(shape)
    return A, B, C0, p


def _gemm_run(device, A, B, C0, M, epi, kg, a_row_off, f16, p):
    return m.debug_codec_gemm(device, A, B, C0, M, epi=epi, kg=kg, a_row_off=a_row_off, bias=p.get("bias"),
                              aux=p.get("aux"), aux2=p.get("aux2"), f=p.get("f", 0), trim=p.get("trim", 0),
                              cout=p.get("cout", 0), rows_out=p.get("rows_out", 0), a_f16=f16)


def _gemm_check(got, ok, want, wr, what):
    assert ok, f"{what}: a guard zone was overwritten"
    gb = got.view(np.uint32)
    assert not np.any(gb[wr] == _SENT32), f"{what}: {int(np.sum(gb[wr] == _SENT32))} elements unwritten"
    assert np.all(gb[~wr] == _SENT32), f"{what}: wrote {int(np.sum(gb[~wr] != _SENT32))} elements outside the contract"
    _check(np.where(wr, got, 0), _Q(np.where(wr, want.val, 0), np.where(wr, want.err, 0)), what)


def _k_values(KG):
    return [32 * KG * j + d for j in (1, 2, 3, 4) for d in (-4, 0, 4)]


@pytest.mark.parametrize("kg,K", [(kg, K) for kg in (0, 1, 2, 4) for K in _k_values(kg or 4)])
def test_gemm_k_stages_and_tails(device, kg, K):
    """STORE + bias at M x N = 129 x 160 (3 x 3 tiles, edge tiles on both sides) over
    K = 32 KG j - 4, 32 KG j, 32 KG j + 4 (j = 1..4): nk = 1..5 stages, both exits of the
    two-stage register ring, with and without a K tail. Bound: the accumulator bound
    (K + 8) u sum|a b| plus the bias add's rounding. Teeth: the reference without its last
    4 k, and the reference with a_row_off off by one, must each fail."""
    M, N = 129, 160
    A, B, C0, p = _gemm_case(_seed("ring", kg, K), M, N, K, m.EPI_STORE)
    got, ok = _gemm_run(device, A, B, C0, M, m.EPI_STORE, kg, 0, 0, p)
    want, wr = _epi_ref(m.EPI_STORE, _gemm_acc(A, B, M), C0, p)
    _gemm_check(got, ok, want, wr, f"kg {kg} K {K}")
    short, _ = _epi_ref(m.EPI_STORE, _gemm_acc(A, B, M, drop=4), C0, p)
    assert _fails(got, short), "the bound does not see 4 dropped k"
    shifted, _ = _epi_ref(m.EPI_STORE, _gemm_acc(A, B, M, a_row_off=1), C0, p)
    assert _fails(got, shifted), "the bound does not see a_row_off + 1"


_GEMM_SHAPES = [(M, N) for M in (1, 31, 33, 64, 65, 129) for N in (32, 64, 96, 160)] + [
    (200, 64),    # tall: m_major = 1, 4 x 1 tiles
    (320, 96),    # tall, m_major = 1, 5 x 2 tiles
    (31, 576),    # wide: 1 x 9 tiles
    (64, 64),     # nb = 1
    (129, 64),    # nb = 3
    (129, 320),   # nb = 15
]


@pytest.mark.parametrize("kg", [0, 1, 2, 4])
@pytest.mark.parametrize("M,N", _GEMM_SHAPES)
def test_gemm_tiles(device, kg, M, N):
    """RESID + bias with C preloaded over M in {1, 31, 33, 64, 65, 129} x N in {32, 64, 96, 160},
    two tall shapes (m_major = 1), a wide one, and tile counts 1, 3, 9, 15 (no multiple of 8:
    the XCD remap leaves idle workgroups); K = 68 KG + 4 (three stages and a tail). The C of a
    residual epilogue is read before the K loop with clamped indices: rows and columns past
    M x N must not be touched (guards)."""
    K = 68 * (kg or 4) + 4
    A, B, C0, p = _gemm_case(_seed("tiles", kg, M, N), M, N, K, m.EPI_RESID)
    got, ok = _gemm_run(device, A, B, C0, M, m.EPI_RESID, kg, 0, 0, p)
    assert ok, "a guard zone was overwritten"
    want, wr = _epi_ref(m.EPI_RESID, _gemm_acc(A, B, M), C0, p)
    assert wr.all()
    _check(got, want, f"kg {kg} {M} x {N}")
    shifted, _ = _epi_ref(m.EPI_RESID, _gemm_acc(A, B, M, a_row_off=1), C0, p)
    assert _fails(got, shifted)


def _convt_variant(f, Kc, snake):
    taps = (Kc + f - 1) // f
    trim = (Kc - f) // 2
    Lin, Cin, Cout = 37, 36, 24
    Lout = f * Lin
    M = (Lout - 1 + trim) // f + 1
    return dict(name=f"convt{'_snake' if snake else ''}_f{f}_k{Kc}", epi=m.EPI_CONVT_SNAKE if snake else m.EPI_CONVT,
                M=M, N=f * Cout, K=taps * Cin, a_seg=Cin, a_rows=Lin, a_row_off=-(taps - 1),
                remap=dict(f=f, trim=trim, cout=Cout, rows_out=Lout))


_EPI_VARIANTS = [
    dict(name="store", epi=m.EPI_STORE, bias=False),
    dict(name="store_bias", epi=m.EPI_STORE),
    dict(name="resid", epi=m.EPI_RESID, bias=False),
    dict(name="resid_bias", epi=m.EPI_RESID),
    dict(name="gated", epi=m.EPI_GATED, bias=False),
    dict(name="swiglu_16", epi=m.EPI_SWIGLU, N=32, bias=False),
    dict(name="swiglu_48", epi=m.EPI_SWIGLU, N=96, bias=False),
    dict(name="swiglu_80", epi=m.EPI_SWIGLU, N=160, bias=False),
    dict(name="snake", epi=m.EPI_SNAKE),
    dict(name="head_17", epi=m.EPI_HEAD, N=64, remap=dict(cout=17)),
    dict(name="head_33", epi=m.EPI_HEAD, N=96, remap=dict(cout=33)),
    dict(name="store_f16", epi=m.EPI_STORE, f16=1),
] + [_convt_variant(f, Kc, snake) for snake in (False, True) for f in (2, 3, 4) for Kc in (f, 2 * f, 2 * f + 1)] + [
    dict(_convt_variant(3, 7, True), name="convt_snake_f16", f16=1),
]


@pytest.mark.parametrize("v", _EPI_VARIANTS, ids=[v["name"] for v in _EPI_VARIANTS])
def test_gemm_epilogues(device, v):
    """Every epilogue under kg = 0 (the launcher's choice), 1, 2 and 4 on the same operands
    (K = 132 where the variant leaves it free: 5, 3 and 2 stages with a tail). STORE / RESID
    with and without bias, GATED, SWIGLU at N/2 = 16, 48, 80 (gate | up rows interleaved per
    16), SNAKE, HEAD at n_freq 17 and 33 (rows interleaved per 16 and padded to 16, ldc =
    2 n_freq, log-magnitudes on both sides of ln 100), and the ConvT remap with and without
    snake for f in {2, 3, 4} x kernel in {f, 2f, 2f + 1} as the decoder forms it (taps =
    ceil(kernel / f), trim = (kernel - f) / 2, a_row_off = -(taps - 1), M = (Lout - 1 + trim) / f
    + 1): rows that map outside [0, rows_out) stay unwritten (three spare sentinel rows after
    rows_out, the guard before row 0). a_f16 = 1 on STORE and CONVT_SNAKE: the reference rounds
    A to f16 first and the unrounded reference must fail.
    Bound: the accumulator bound carried through the epilogue's own f32 operations (_Q).
    The three K-group counts add their chains in different orders: they must agree within
    twice the bound, not bit for bit."""
    epi, f16 = v["epi"], v.get("f16", 0)
    M, N, K = v.get("M", 65), v.get("N", 96), v.get("K", 132)
    off, remap = v.get("a_row_off", 0), v.get("remap", {})
    A, B, C0, p = _gemm_case(_seed("epi", v["name"]), M, N, K, epi, a_row_off=off, a_rows=v.get("a_rows"),
                             a_seg=v.get("a_seg"), f16=f16, bias=v.get("bias", True), **remap)
    want, wr = _epi_ref(epi, _gemm_acc(A, B, M, off, f16), C0, p)
    if epi == m.EPI_HEAD:
        lm = _gemm_acc(A, B, M).val[:, :16] + p["bias"][:16]
        assert (lm > np.log(100.0) + 1).any() and (lm < np.log(100.0) - 1).any()
    outs = {}
    for kg in (0, 1, 2, 4):
        got, ok = _gemm_run(device, A, B, C0, M, epi, kg, off, f16, p)
        _gemm_check(got, ok, want, wr, f"{v['name']} kg {kg}")
        outs[kg] = np.where(wr, got, 0).astype(np.float64)
        shifted, _ = _epi_ref(epi, _gemm_acc(A, B, M, off + 1, f16), C0, p)
        assert _fails(np.where(wr, got, 0), _Q(np.where(wr, shifted.val, 0), np.where(wr, shifted.err, 0)))
        if f16:
            unrounded, _ = _epi_ref(epi, _gemm_acc(A, B, M, off, False), C0, p)
            assert _fails(np.where(wr, got, 0), _Q(np.where(wr, unrounded.val, 0), np.where(wr, unrounded.err, 0))), \
                "the bound does not see A left unrounded"
    for a, b in ((1, 2), (1, 4), (2, 4)):
        assert np.all(np.abs(outs[a] - outs[b]) <= 2 * np.where(wr, want.err, 0)), (a, b)
    assert np.array_equal(outs[0], outs[4])  # 6 tiles at most: the launcher picks 4 K-groups


def test_gemm_refuses_unaligned_k(device):
    """K % 4 and a_seg % 4 are preconditions of the float4 operand loads (codec_kernels.h): the
    entry point refuses them instead of launching."""
    A, B = np.zeros((8, 34), np.float32), np.zeros((32, 34), np.float32)
    with pytest.raises(m.HipError):
        m.debug_codec_gemm(device, A, B, m.sentinel_f32((8, 32)), 8)


def test_epilogue_function_allowance(device):
    """expf, sinf and cosf as the epilogues call them, on accumulators that are exact: K = 8
    with B rows (1, 0, ..) for the log-magnitude columns and (0, 0, 0, 0, 1, 0, ..) for the phase
    columns makes the HEAD epilogue (bias 0) return clamp(expf(A[m][0])) cosf(A[m][4]) and
    .. sinf(A[m][4]). A[m][4] = 0 isolates expf (cosf(0) = 1, sinf(0) = 0), A[m][0] = 0
    isolates cosf and sinf (expf(0) = 1). Arguments: v in [-30, ln 100), p in [-100, 100] and
    [-3.2, 3.2], the range the N(0, 1) GEMM tests produce. The deviations from float64 are
    printed in units of 2^-23 and must stay inside the allowances. Measured on the MI355X:
    expf 0.544 (allowance 2), cosf 0.435 and sinf 0.443 (allowance 1 each)."""
    M = 512
    rng = _seed("ulp")
    B8 = np.zeros((32, 8), np.float32)
    B8[:16, 0] = 1.0
    B8[16:, 4] = 1.0
    bias = np.zeros(32, np.float32)

    def head(col, x32):
        A = np.zeros((M, 8), np.float32)
        A[:, col] = x32
        got, ok = m.debug_codec_gemm(device, A, B8, m.sentinel_f32((M, 32)), M, epi=m.EPI_HEAD, kg=0, bias=bias,
                                     cout=16)
        assert ok and not np.any(got.view(np.uint32) == _SENT32)
        return got.astype(np.float64)

    worst = {}
    v32 = _f32(rng.uniform(-30.0, np.log(100.0) - 1e-3, M))
    got = head(0, v32)
    ex = np.exp(v32.astype(np.float64))[:, None]
    assert np.all(got[:, 1::2] == 0)
    worst["exp"] = float(np.max(np.abs(got[:, 0::2] - ex) / ex) / 2.0 ** -23)
    for name, lim in (("wide", 100.0), ("narrow", 3.2)):
        p32 = _f32(rng.uniform(-lim, lim, M))
        got = head(4, p32)
        x = p32.astype(np.float64)[:, None]
        worst["cos_" + name] = float(np.max(np.abs(got[:, 0::2] - np.cos(x))) / 2.0 ** -23)
        worst["sin_" + name] = float(np.max(np.abs(got[:, 1::2] - np.sin(x))) / 2.0 ** -23)
    print("measured deviation from float64, units of 2^-23:", worst)
    assert worst["exp"] <= _E_EXP
    assert max(worst["cos_wide"], worst["cos_narrow"]) <= _E_COS
    assert max(worst["sin_wide"], worst["sin_narrow"]) <= _E_SIN


# ------------------------------------------------------------------------------ conv f16
def _conv_ref(xa, w, bias, taps, pad, resid, shift=0, drop=0):
    L, Cin = xa.shape
    K = taps * Cin
    X = np.zeros((L + 2 * taps + 2, Cin))
    X[taps + 1:taps + 1 + L] = xa.astype(np.float64)
    rows = np.arange(L)[:, None] - pad + shift + np.arange(taps)[None, :] + taps + 1
    W = X[rows].reshape(L, K)   # [l][tap * Cin + ci]
    w64 = w.astype(np.float64)
    acc = _dot(W[:, :K - drop], w64[:, :K - drop], K)
    y = acc + _Q(bias)
    return y + _Q(resid) if resid is not None else y


_CONV_CASES = [
    # taps, Cin, Cout, L            K = taps * Cin -> 128-deep stages
    (1, 8, 8, 1),        # nk 1, one 8-chunk
    (1, 64, 72, 63),     # nk 1
    (3, 8, 130, 2),      # nk 1, K = 24
    (3, 24, 64, 64),     # nk 1, K = 72
    (3, 64, 8, 65),      # nk 2, K = 192
    (5, 24, 72, 130),    # nk 1, K = 120 (8 short of a stage)
    (5, 64, 130, 65),    # nk 3, K = 320
    (3, 72, 64, 63),     # nk 2, K = 216: an 8-wide tail past 208
    (5, 72, 72, 64),     # nk 3, K = 360: 256 + 104 (an 8-wide tail)
    (3, 512, 130, 130),  # nk 12, 3 x 3 tiles
    (1, 512, 64, 1),     # nk 4
]


@pytest.mark.parametrize("resid", ["none", "separate", "alias"])
@pytest.mark.parametrize("taps,Cin,Cout,L", _CONV_CASES)
def test_conv_f16(device, taps, Cin, Cout, L, resid):
    """conv_f16_kernel with taps 1, 3, 5 (pad = taps / 2), Cin in {8, 24, 64, 72, 512}, Cout in
    {8, 64, 72, 130}, L in {1, 2, 63, 64, 65, 130}: 1, 2, 3, 4 and 12 K stages, stages that end
    in an 8-wide tail, edge tiles in both directions; residual absent, in a buffer of its own,
    and aliasing Y. Both operands are f16, so every product is exact in f32 and the bound is the
    accumulator bound (K + 8) u sum|x w| plus one rounding each for the bias and residual adds.
    Teeth: the padding shifted by one row, and the last 8-chunk of K dropped."""
    rng = _seed("conv", taps, Cin, Cout, L)
    xa = rng.standard_normal((L, Cin)).astype(np.float16)
    w = rng.standard_normal((Cout, taps * Cin)).astype(np.float16)
    bias = _f32(rng.standard_normal(Cout))
    r = None if resid == "none" else _f32(rng.standard_normal((L, Cout)))
    got, ok = m.debug_codec_conv(device, xa, w, bias, taps, taps // 2, resid=r, alias=resid == "alias")
    _check(got, _conv_ref(xa, w, bias, taps, taps // 2, r), f"conv {taps} {Cin} {Cout} {L} {resid}", ok)
    assert _fails(got, _conv_ref(xa, w, bias, taps, taps // 2, r, shift=1)), "padding shifted by a row passes"
    assert _fails(got, _conv_ref(xa, w, bias, taps, taps // 2, r, drop=8)), "a dropped 8-chunk of K passes"


# ------------------------------------------------------------------------------ row norm
def _rownorm_ref(x, eps, mode, p0, p1):
    """rownorm_kernel: the sums in double (error ~2^-53, inside _TINY's company: carried as
    one f32 rounding of the mean and of the variance), everything else in f32."""
    x64 = x.astype(np.float64)
    mean = _mean_f32(x64.mean(axis=1, keepdims=True))
    d = _Q(x64) - mean
    sq = d * d
    var = _Q(sq.val.mean(axis=1, keepdims=True), sq.err.mean(axis=1, keepdims=True)).f32()
    scale = _Q(1.0) / (var + _Q(np.float64(np.float32(eps)))).sqrt()
    t = d * scale
    if mode == 1:
        t = t * _Q(p0)
        if p1 is not None:
            t = t + _Q(p1)
    elif mode == 2:
        t = t * (_Q(1.0) + _Q(p1)) + _Q(p0)
    return t


@pytest.mark.parametrize("D", list(range(64, 1025, 64)))
def test_rownorm(device, D):
    """rownorm_kernel<D / 64> for all 16 widths, M in {1, 3, 4, 5, 9} (four rows per
    workgroup: partial and multiple workgroups), mode 0, mode 1 with and without b, mode 2,
    out of place and in place. Bound (derived, not fitted): mean and variance are double sums
    cast to f32 (one rounding each); d = x - mean, d * d, variance + eps, sqrtf, 1 / s,
    d * scale and the affine steps are one f32 rounding each, carried by _Q. For N(0, 1) rows
    this is ~6 u |y| ~ 4e-7 |y|, asserted below to be 100x under the 1e-3 stage bar."""
    eps = 1e-5
    for M in (1, 3, 4, 5, 9):
        rng = _seed("rownorm", D, M)
        x = _f32(rng.standard_normal((M, D)) + 0.3)
        w, b = _f32(1 + 0.5 * rng.standard_normal(D)), _f32(rng.standard_normal(D))
        sh, sc = _f32(rng.standard_normal(D)), _f32(0.5 * rng.standard_normal(D))
        for mode, p0, p1 in ((0, None, None), (1, w, b), (1, w, None), (2, sh, sc)):
            want = _rownorm_ref(x, eps, mode, p0, p1)
            _assert_tight(want)
            for in_place in (False, True):
                got, ok = m.debug_codec_rownorm(device, x, eps, mode, p0, p1, in_place)
                _check(got, want, f"rownorm D {D} M {M} mode {mode} in_place {in_place}", ok)
        # teeth: a reference normalized by D - 1 instead of D
        wrong = _rownorm_ref(x, eps, 0, None, None)
        wrong = _Q(wrong.val * np.sqrt((D - 1) / D), wrong.err)
        got, ok = m.debug_codec_rownorm(device, x, eps, 0)
        assert _fails(got, wrong)


# ------------------------------------------------------------------------------ group norm
_GN_CG = [(64, 8), (512, 32), (1024, 64), (64, 64), (72, 9), (136, 17), (1024, 16)]
_GN_L = [1, 3, 4, 5, 511, 513, 1030]
_GN_EPS = 1e-6


def _gn_inputs(C, G, L):
    rng = _seed("gn", C, G, L)
    x = _f32(rng.standard_normal((L, C)) + 0.25 * rng.standard_normal((1, C)))
    gamma = _f32(1 + 0.3 * rng.standard_normal(C))
    beta = _f32(0.5 * rng.standard_normal(C))
    return x, gamma, beta


def _gn_ref(x, G, gamma, beta):
    """The value before the f16 rounding and the bound delta on the f32 value the kernel
    rounds: group statistics are double sums cast to f32 (mean; variance of the f32
    fl(fl(x - mean)^2)), then (x - mean) * rstd * gamma + beta and silu in f32."""
    L, C = x.shape
    cpg = C // G
    xg = x.astype(np.float64).reshape(L, G, cpg)
    mean = _mean_f32(xg.mean(axis=(0, 2), keepdims=True))
    d = _Q(xg) - mean
    sq = d * d
    var = _Q(sq.val.mean(axis=(0, 2), keepdims=True), sq.err.mean(axis=(0, 2), keepdims=True)).f32()
    rstd = _Q(1.0) / (var + _Q(np.float64(np.float32(_GN_EPS)))).sqrt()
    y = d * rstd
    y = _Q(y.val.reshape(L, C), y.err.reshape(L, C))
    y = y * _Q(gamma) + _Q(beta)
    return _silu(y)


def _gn_check(got, want: _Q, ok, what):
    """Exact check of an f16 output: every element equals the f16 rounding r of the float64
    value, or is the f16 neighbour of r on the side where the float64 value lies within delta
    of the rounding boundary between the two. Anything else fails (two f16 ulps included)."""
    assert ok, f"{what}: a guard zone was overwritten"
    assert not np.any(got.view(np.uint16) == _SENT16), f"{what}: unwritten elements"
    inf = np.float16(np.inf)
    with np.errstate(over="ignore"):
        r = want.val.astype(np.float16)
    dn, up = np.nextafter(r, -inf), np.nextafter(r, inf)
    r64, dn64, up64 = r.astype(np.float64), dn.astype(np.float64), up.astype(np.float64)
    near_dn = want.val - want.err <= 0.5 * (r64 + dn64)   # boundary below r within delta
    near_up = want.val + want.err >= 0.5 * (r64 + up64)
    good = (got == r) | ((got == dn) & near_dn) | ((got == up) & near_up)
    assert np.all(good), (f"{what}: {int((~good).sum())} of {good.size} elements off; first "
                          f"{np.argwhere(~good)[0]}: got {got[~good][0]!r} want {r[~good][0]!r} "
                          f"(float64 {want.val[~good][0]!r}, delta {want.err[~good][0]:.3g})")
    return int(np.sum(got != r))


@pytest.mark.parametrize("C,G", _GN_CG)
def test_groupnorm_default_pipeline(device, C, G):
    """MIO_GN = 3 (gn_partial<1> + gn_stat2 + gn_apply3) over (C, G) with 4 and 8 group
    rounds per reduction (G <= 32 / G > 32), C / G from 1 to 64, C no multiple of 64 (72, 136:
    a partial last 64-channel slice), and L in {1, 3, 4, 5, 511, 513, 1030} around the switch
    from 4 rows per slice to more at L = 512. The output is f16: the check is exact (see
    _gn_check), with delta from _gn_ref. Teeth: the population variance replaced by the sample
    variance must fail where the group has few enough elements for it to show."""
    assert os.environ.get("MIO_GN", "3") == "3"
    for L in _GN_L:
        x, gamma, beta = _gn_inputs(C, G, L)
        got, ok = m.debug_codec_groupnorm(device, x, G, _GN_EPS, gamma, beta)
        want = _gn_ref(x, G, gamma, beta)
        _gn_check(got, want, ok, f"gn C {C} G {G} L {L}")
        n = L * (C // G)
        if 1 < n <= 256:
            xs = (x.astype(np.float64).reshape(L, G, C // G))
            mu = xs.mean(axis=(0, 2), keepdims=True)
            y = ((xs - mu) / np.sqrt(xs.var(axis=(0, 2), keepdims=True, ddof=1) + _GN_EPS)).reshape(L, C) * gamma + beta
            wrong = _Q(y / (1 + np.exp(-y)), want.err)
            with pytest.raises(AssertionError):
                _gn_check(got, wrong, ok, "teeth")


_GN_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import miotts_amd as m
dev = m.Device(0)
src = np.load(sys.argv[2])
out = {}
for key in src.files:
    if not key.startswith("x_"):
        continue
    tag = key[2:]
    G = int(tag.split("_")[1])
    xa, ok = m.debug_codec_groupnorm(dev, src[key], G, float(src["eps"]), src["g_" + tag], src["b_" + tag])
    out["y_" + tag] = xa.view(np.uint16)
    out["ok_" + tag] = np.array(ok)
np.savez(sys.argv[3], **out)
dev.close()
"""


@pytest.mark.parametrize("mode", [1, 5])
def test_groupnorm_other_pipelines(device, tmp_path, mode):
    """MIO_GN = 1 (gn_fused_kernel where C / G is 4, 8, 16, 32 or 64, the sliced five launches
    otherwise) and MIO_GN = 5 (gn_partial<1|2> + gn_final<1|2> + gn_apply) ship behind the
    switch and meet the same exact check on the same cases. The switch is read once per
    process, so each mode runs in a fresh child."""
    cases = [(C, G, L) for C, G in _GN_CG for L in _GN_L]
    arrays = {"eps": np.float32(_GN_EPS)}
    for C, G, L in cases:
        x, gamma, beta = _gn_inputs(C, G, L)
        arrays[f"x_{C}_{G}_{L}"], arrays[f"g_{C}_{G}_{L}"], arrays[f"b_{C}_{G}_{L}"] = x, gamma, beta
    src, dst, script = tmp_path / "in.npz", tmp_path / "out.npz", tmp_path / "gn_child.py"
    np.savez(src, **arrays)
    script.write_text(_GN_CHILD)
    pkg = os.path.dirname(os.path.dirname(m.__file__))
    p = subprocess.run([sys.executable, str(script), pkg, str(src), str(dst)], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, MIO_GN=str(mode)))
    assert p.returncode == 0, p.stderr[-2000:]
    out = np.load(dst)
    for C, G, L in cases:
        tag = f"{C}_{G}_{L}"
        want = _gn_ref(arrays["x_" + tag], G, arrays["g_" + tag], arrays["b_" + tag])
        _gn_check(out["y_" + tag].view(np.float16), want, bool(out["ok_" + tag]), f"MIO_GN {mode} C {C} G {G} L {L}")


# ------------------------------------------------------------------------------ band attention
def _rope_f32(x, cs):
    """The kernel's roped row, bit for bit: (x0 c - x1 s, x0 s + x1 c) with each product and
    each sum rounded to f32 once (contraction is off in codec_kernels.hip). IEEE f32 multiply,
    add and subtract are deterministic, so numpy's f32 gives the device's values and the
    float64 reference starts from them, as the a_f16 GEMM reference starts from the rounded A."""
    x = x.astype(np.float32)
    x0, x1, c, s = x[..., 0::2], x[..., 1::2], cs[..., 0].astype(np.float32), cs[..., 1].astype(np.float32)
    out = np.empty(x.shape, np.float32)
    out[..., 0::2] = (x0 * c) - (x1 * s)
    out[..., 1::2] = (x0 * s) + (x1 * c)
    return out.astype(np.float64)


def _band_ref(qkv, H, hw, rope):
    """softmax(q k^T / 8 over |i - j| <= hw) v per head in float64 from the roped f32 rows
    (_rope_f32), with the bound of the kernel's order:
      * a score is one ascending-d chain of 64 fmaf, each rounding its partial sum once:
        u sum_d |partial_d| (tighter than 64 u sum|q k|), scaled by 1/8 exactly;
      * w_i = expf(s_i - max): relative error r_i = the score's error + the subtraction's
        rounding + the expf allowance (the maximum shifts every exponent of a row alike and
        cancels below);
      * the sum of <= 65 w is at most 5 sequential adds and a 4-level tree (9 roundings), then
        1 / sum and p_i = w_i * inv: a common relative factor kappa <= 11 u and one more u per
        p_i. So p_i(device) = p_i (1 + r_i) (1 + kappa) / sum_j p_j (1 + r_j), and to first
        order out_d(device) - out_d = sum_i p_i r_i (v_id - out_d) + kappa out_d: only the
        spread of v around the output carries the weights' errors (second order: factor
        1 + 4 max r);
      * the output is one ascending-j fmaf chain over the band: u sum_j |partial_j|."""
    S = qkv.shape[0]
    D = H * 64
    val, err = np.zeros((S, D)), np.zeros((S, D))
    i, j = np.arange(S)[:, None], np.arange(S)[None, :]
    band = np.abs(i - j) <= hw
    for h in range(H):
        q = _rope_f32(qkv[:, h * 64:(h + 1) * 64], rope)
        k = _rope_f32(qkv[:, D + h * 64:D + (h + 1) * 64], rope)
        v = qkv[:, 2 * D + h * 64:2 * D + (h + 1) * 64].astype(np.float64)
        part = np.cumsum(q[:, None, :] * k[None, :, :], axis=2)
        s = _Q(part[:, :, -1] * 0.125, _U * np.abs(part).sum(axis=2) * (1 + 64 * _U) * 0.125)
        mx = np.max(np.where(band, s.val, -np.inf), axis=1, keepdims=True)
        w = (s - _Q(mx)).exp()
        wv = np.where(band, w.val, 0.0)
        r = np.where(band, w.err / np.where(band, w.val, 1.0) + _U, 0.0)
        pv = wv / wv.sum(axis=1, keepdims=True)
        opart = np.cumsum(pv[:, :, None] * v[None, :, :], axis=1)
        out = opart[:, -1, :]
        spread = np.einsum("ij,ijd->id", pv * r, np.abs(v[None, :, :] - out[:, None, :]))
        val[:, h * 64:(h + 1) * 64] = out
        err[:, h * 64:(h + 1) * 64] = ((spread + 11 * _U * np.abs(out)) * (1 + 4 * r.max())
                                       + _U * np.abs(opart).sum(axis=1) * (1 + 65 * _U) + _TINY)
    return _Q(val, err)


@pytest.mark.parametrize("window", [1, 3, 17, 65])
@pytest.mark.parametrize("H", [1, 2, 3])
def test_band_attention(device, H, window):
    """band_attention_kernel at half widths 0, 1, 8, 32 and S in {1, 2, 15, 16, 17, 33, 100}
    around its 16-query blocks (a partial block, exactly one, one query more, several), 1-3
    heads, random unit (cos, sin) rotations. Bound: _band_ref. Against the stage bar it comes
    out >= 100x tighter at every size in the max form (<= 1.3e-5 of the largest value against
    5e-3) and in the RMS form up to window 17; at window 65 the RMS of the bound is 1.1e-5
    (S = 33) to 1.5e-5 (S = 100) of the RMS of the output, 70x under 1e-3: a worst-case score
    error of u sum|partial| / 8 ~ 2.5e-6 weighs sum p |v - out| ~ 0.85 while the output of 65
    averaged N(0, 1) rows has RMS ~ 0.23, and no order of roundings makes that ratio smaller.
    Teeth: the reference with half width + 1 must fail
    wherever that admits another key (S > hw + 1)."""
    hw = window // 2
    for S in (1, 2, 15, 16, 17, 33, 100):
        rng = _seed("band", H, window, S)
        qkv = _f32(rng.standard_normal((S, 3 * H * 64)))
        ang = rng.uniform(-np.pi, np.pi, (S, 32))
        rope = _f32(np.stack([np.cos(ang), np.sin(ang)], axis=-1))
        got, ok = m.debug_codec_band_attention(device, qkv, H, window, rope)
        want = _band_ref(qkv, H, hw, rope)
        _assert_tight(want, 1e-5 if window < 65 else 1.5e-5)
        _check(got, want, f"band S {S} H {H} window {window}", ok)
        if S > hw + 1:
            assert _fails(got, _band_ref(qkv, H, hw + 1, rope)), f"S {S}: half width + 1 passes"


# ------------------------------------------------------------------------------ cond GEMV, embed
@pytest.mark.parametrize("e_f16", [0, 1])
def test_cond_gemv(device, e_f16):
    """cond_gemv_kernel over R in {1, 3, 4, 5, 384} (four rows per workgroup) x A in {1, 63, 64,
    65, 200} (lane-strided: fewer terms than lanes, exactly 64, a second round). Bound: silu in
    f32 (_silu); each lane's fmaf chain of ceil(A / 64) terms, a 6-level tree and the bias add:
    (ceil(A / 64) + 7) u sum|W silu(e)| plus sum|W| e_silu. With e_f16 the reference rounds
    silu(e) to f16 as the kernel does (an element whose float64 value lies within its f32
    error of an f16 rounding boundary may round either way: one f16 ulp is allowed there), and
    the unrounded reference must fail."""
    for R in (1, 3, 4, 5, 384):
        for A in (1, 63, 64, 65, 200):
            rng = _seed("gemv", R, A)
            W, b, e = _f32(rng.standard_normal((R, A))), _f32(rng.standard_normal(R)), _f32(rng.standard_normal(A))
            got, ok = m.debug_codec_cond_gemv(device, W, b, e, e_f16)

            def ref(rounded):
                se = _silu(_Q(e.astype(np.float64)))
                if rounded:
                    r = se.val.astype(np.float16)
                    amb = ((se.val - se.err).astype(np.float16) != r) | ((se.val + se.err).astype(np.float16) != r)
                    se = _Q(r.astype(np.float64), np.where(amb, np.spacing(np.abs(r)).astype(np.float64), 0.0))
                W64 = W.astype(np.float64)
                acc = _Q(W64 @ se.val, ((A + 63) // 64 + 7) * _U * (np.abs(W64) @ np.abs(se.val)) + np.abs(W64) @ se.err)
                return acc + _Q(b)

            want = ref(e_f16)
            if R == 384:   # a few rows alone may cancel to a small value: judged on the full matrix
                _assert_tight(want)
            _check(got, want, f"cond_gemv R {R} A {A} e_f16 {e_f16}", ok)
            if e_f16 and R * A >= 64:
                assert _fails(got, ref(False)), f"R {R} A {A}: the unrounded reference passes"


def test_embed(device):
    """embed_kernel copies table rows bit for bit: T = 1, duplicate codes, first and last row,
    widths of one float4 up to 1024 (payload NaNs and negative zeros included)."""
    rng = _seed("embed")
    for D in (4, 64, 200, 1024):
        table = rng.integers(0, 2 ** 32, (37, D), dtype=np.uint64).astype(np.uint32).view(np.float32)
        for codes in ([5], [0, 36, 36, 0, 7, 7, 7], list(rng.integers(0, 37, 70))):
            got, ok = m.debug_codec_embed(device, table, codes)
            assert ok
            assert np.array_equal(got.view(np.uint32), table.view(np.uint32)[np.asarray(codes)]), (D, codes)
    with pytest.raises(m.HipError):
        m.debug_codec_embed(device, table, [37])
