"""CPU: the joint row reduction's float tree (llm_device.h rows_joint: row_ror:8, then the two
permlane swaps, over values replicated in half groups) gives the float32 bits of sum_lanes7's
tree (row_shr:8, row_bcast:15, row_bcast:31 to lane 63), and every row's totals end in the lanes
its epilogue reads them from. Both are modelled lane by lane in numpy float32; a wrong pairing
or a wrong lane shows here without a GPU."""
import numpy as np
import pytest

F = np.float32


def _old_total(t):
    """sum_lanes7 on the 8 superblock terms t[k] held in lanes 8k + 7 (other lanes: junk)."""
    v = np.full(64, F(123.25))
    v[7::8] = t
    lanes = np.arange(64)
    # row_shr:8, old = 0: lane l of a row gets lane l - 8 (0 where l < 8)
    src = np.where(lanes % 16 >= 8, v[np.maximum(lanes - 8, 0)], F(0))
    v = (v + src).astype(F)
    # row_bcast:15, row_mask 0xA: rows 1 and 3 add lane 15 of the row before
    src = np.where((lanes // 16) % 2 == 1, v[np.maximum(16 * (lanes // 16) - 1, 0)], F(0))
    v = (v + src).astype(F)
    # row_bcast:31, row_mask 0xC: rows 2 and 3 add lane 31
    src = np.where(lanes >= 32, v[31], F(0))
    v = (v + src).astype(F)
    return v[63]


def _ror8_add(v):
    lanes = np.arange(64)
    return (v + v[(lanes & ~15) | ((lanes + 8) & 15)]).astype(F)


def _swap16(a, b):
    """v_permlane16_swap: odd rows of a (vdst) exchanged with even rows of b (src0)."""
    a, b = a.copy(), b.copy()
    for r in (0, 2):
        lo, hi = slice(16 * r, 16 * r + 16), slice(16 * r + 16, 16 * r + 32)
        a[hi], b[lo] = b[lo].copy(), a[hi].copy()
    return a, b


def _swap32(a, b):
    """v_permlane32_swap: the upper half of a (vdst) exchanged with the lower half of b (src0)."""
    a, b = a.copy(), b.copy()
    a[32:], b[:32] = b[:32].copy(), a[32:].copy()
    return a, b


def _swapadd(swap, a, b):
    r0, r1 = swap(a, b)
    return (r1 + r0).astype(F)


def _pair_lanes(ta, tb):
    """The per-lane value after pair_term: superblock (lane >> 3)'s term of unit A in the lanes
    with bit 2 clear, of unit B in the others, plus the row's first add to 0."""
    lanes = np.arange(64)
    v = np.where(lanes & 4, tb[lanes >> 3], ta[lanes >> 3]).astype(F)
    return (F(0) + v).astype(F)


def _shl4(v):
    lanes = np.arange(64)
    return np.where(lanes % 16 < 12, v[np.minimum(lanes + 4, 63)], F(0)).astype(F)


def _joint_nm2(t):
    """t[row][matrix][8] -> {row: (dot0, dot1)} as rows_joint<NM = 2> leaves them for fin."""
    n = len(t)
    x = [_ror8_add(_pair_lanes(t[p][0], t[p][1])) for p in range(n)]
    if n <= 2:
        q = _swapadd(_swap16, x[0], x[n - 1])
        r = _swapadd(_swap32, q, q)
    else:
        q, q2 = _swapadd(_swap16, x[0], x[1]), _swapadd(_swap16, x[2], x[n - 1])
        r = _swapadd(_swap32, q, q2)
    r1 = _shl4(r)
    return {p: (r[16 * p], r1[16 * p]) for p in range(n)}


def _joint_nm1(t):
    """t[row][8] -> {row: dot} as rows_joint<NM = 1> parks them (row u in lane u)."""
    su = len(t)
    p0 = np.zeros(64, F)
    for p in range((su + 1) // 2):
        b = min(2 * p + 1, su - 1)
        x = _ror8_add(_pair_lanes(t[2 * p], t[b]))
        q = _swapadd(_swap16, x, x)
        r = _swapadd(_swap32, q, q)
        rs = _shl4(r)
        for u in range(2 * p, min(2 * p + 2, su)):
            v = r if ((u >> 2) & 1) == (u & 1) else rs
            p0[u] = v[u]
    return {u: p0[u] for u in range(su)}


def _terms(rng, kind, shape):
    if kind == "random":
        return (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 6, shape)).astype(F)
    if kind == "cancelling":  # large terms that cancel down to the small ones' scale
        t = rng.standard_normal(shape).astype(F)
        big = (rng.standard_normal(shape[:-1] + (4,)) * 1e7).astype(F)
        t[..., :4] += big
        t[..., 4:] -= big[..., ::-1]
        return t
    t = np.zeros(shape, F)  # signed zeros: the first add to 0.0 turns -0.0 into +0.0
    t[..., ::2] = F(-0.0)
    return t


def _same(a, b):
    return np.asarray(a, F).view(np.uint32) == np.asarray(b, F).view(np.uint32)


@pytest.mark.parametrize("kind", ["random", "cancelling", "zeros"])
@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_joint_tree_row_pairs(kind, rows):
    rng = np.random.default_rng(7 + rows)
    for _ in range(50):
        t = _terms(rng, kind, (rows, 2, 8))
        got = _joint_nm2(t)
        for p in range(rows):
            want = [_old_total((F(0) + t[p][m]).astype(F)) for m in range(2)]
            assert _same(got[p][0], want[0]) and _same(got[p][1], want[1]), (kind, rows, p)


@pytest.mark.parametrize("kind", ["random", "cancelling", "zeros"])
@pytest.mark.parametrize("su", [2, 3, 4, 6, 8])
def test_joint_tree_rows(kind, su):
    rng = np.random.default_rng(70 + su)
    for _ in range(50):
        t = _terms(rng, kind, (su, 8))
        got = _joint_nm1(t)
        for u in range(su):
            assert _same(got[u], _old_total((F(0) + t[u]).astype(F))), (kind, su, u)


def test_tree_shape_matters():
    """The check can fail: a left-to-right sum of the same terms differs in some draw."""
    rng = np.random.default_rng(1)
    t = _terms(rng, "cancelling", (200, 8))
    seq = np.zeros(200, F)
    for k in range(8):
        seq = (seq + t[:, k]).astype(F)
    assert any(not _same(seq[i], _old_total(t[i])) for i in range(200))
