"""CPU: tests/np_rowdot.py checked against itself and against independent code - the encoders
against np_ref.dequant (and the host dequantizer where the library loads), the reference against
the float64 dot of the dequantized operands, the unmutated per-lane model against the bound on
every (type, weight case, activation case, k), and every mutant caught by at least one of them.
"""
import itertools

import numpy as np
import pytest

import np_act_quant as aq
import np_q5k
import np_ref
import np_rowdot as rd

ROWS = 17  # every sub-block of one_field (16 for Q6_K), every ceiling variant (8 for Q6_K)


def _lib():
    try:
        import miotts_amd as m
        m.lib()
        return m
    except Exception:  # noqa: BLE001 - no library on this machine: the numpy checks still run
        return None


def _combos(qtype):
    return itertools.product(rd.WEIGHT_CASES, rd.ACT_CASES, rd.WIDTHS[qtype])


def _dequant_act(qtype, x):
    if qtype == 30:
        return np_ref.act_bf16(x)
    if qtype == 8:
        q, d = aq.q8_0(x)
        return (q.astype(np.float64).reshape(-1, 32) * d.astype(np.float64)[:, None]).reshape(-1)
    q, d, _ = aq.q8_k(x)
    return (q.astype(np.float64).reshape(-1, 256) * d.astype(np.float64)[:, None]).reshape(-1)


@pytest.mark.parametrize("qtype", rd.TYPES)
def test_encoder_decoder_identity(qtype):
    """Every weight case decoded by np_ref.dequant (np_q5k's for type 13) equals the fields, and
    the bytes decode back to the fields; mio_dequantize_rows agrees to float32 rounding."""
    m = _lib()
    for case, k in itertools.product(rd.WEIGHT_CASES, rd.WIDTHS[qtype]):
        f, raw = rd.weight_case(qtype, case, ROWS, k)
        want = rd.values(qtype, f)
        assert np.all(np.isfinite(want)), (case, k)
        got = np_q5k.dequant(qtype, raw.reshape(-1), ROWS, k) if qtype == 13 else np_ref.dequant(qtype, raw.reshape(-1), ROWS, k)
        if qtype == 13:  # ggml's float32 expression order: three roundings of values below 2^28
            assert np.all(np.abs(got - want) <= 3 * 2.0 ** -24 * (np.abs(want) + np.abs(got)) + 1e-30), (case, k)
        else:
            assert np.array_equal(got, want), (case, k)
        back = rd.decode_fields(qtype, raw, ROWS, k)
        for key, v in f.items():
            assert np.array_equal(np.asarray(back[key]).view(np.uint16) if key in ("d", "dmin") else back[key],
                                  np.asarray(v).view(np.uint16) if key in ("d", "dmin") else v), (case, k, key)
        if m is not None:
            host = m.dequantize_rows(qtype, raw, k).astype(np.float64)
            assert np.all(np.abs(host - want) <= 4 * 2.0 ** -24 * np.abs(want) + 2.0 ** -126), (case, k)


def test_q5k_encoder_equals_np_q5k():
    f, raw = rd.weight_case(13, "random_bytes", 5, 768)
    for r, b in itertools.product(range(5), range(3)):
        blk = np_q5k.pack_block(f["d"][r, b], f["dmin"][r, b], f["sc"][r, b], f["mn"][r, b], f["q"][r, b])
        assert np.array_equal(blk, raw[r, 176 * b:176 * (b + 1)]), (r, b)


@pytest.mark.parametrize("qtype", (2, 6))
def test_repacked_types_decode_as_q8_0(qtype):
    rng = np.random.default_rng(qtype)
    raw = rng.integers(0, 256, (9, 576 // 32 * rd.BLOCK[qtype][1])).astype(np.uint8)
    raw.reshape(9, -1, rd.BLOCK[qtype][1])[..., 1] &= 0x3F  # a finite d
    f = rd.decode_fields(qtype, raw, 9, 576)
    assert np.array_equal(rd.values(qtype, f), np_ref.dequant(qtype, raw.reshape(-1), 9, 576))
    assert f["q"].min() >= -16 and f["q"].max() <= 15


def _block_dots(qtype, w, x):
    """float64 [R, nb]: the dot of every activation block with the dequantized weights under it,
    its integer part exact. A float64 `@` will not do: S_abs counts a block's integer sum AFTER
    its cancellation (the alternating activation cancels the mins exactly), so the products'
    own roundings would pass 1e-12 S_abs. Every weight is a multiple of 2^-24 below 2^28: split
    into two 26-bit halves, both integer sums against the int8 codes are exact in int64."""
    if qtype == 8:
        qa, da = aq.q8_0(x)
    else:
        qa, da, _ = aq.q8_k(x)
    blk = rd.act_blk(qtype)
    wi = np.rint(w * 2.0 ** 24)
    assert np.array_equal(wi, w * 2.0 ** 24) and np.abs(wi).max() < 2.0 ** 52
    wi = wi.astype(np.int64).reshape(w.shape[0], -1, blk)
    hi = wi >> 26
    lo = wi - (hi << 26)
    qa = qa.astype(np.int64).reshape(-1, blk)
    s = (hi * qa).sum(-1).astype(object) * (1 << 26) + (lo * qa).sum(-1).astype(object)
    return s.astype(np.float64) * da.astype(np.float64) * 2.0 ** -24


@pytest.mark.parametrize("qtype", rd.TYPES)
def test_reference_identity(qtype):
    """y_ref = dequant(w) . dequant(a) to 1e-12 of S_abs, with np_ref's decoder (np_q5k's codes
    for type 13) and the quantized activation's codes; |x| <= 1e3."""
    for case, act, k in _combos(qtype):
        f, raw = rd.weight_case(qtype, case, ROWS, k)
        x = rd.act_case(act, k, rd.act_blk(qtype))
        assert np.abs(x).max() <= 1e3
        y, s_abs, _, _ = rd.reference(qtype, f, x, k)
        if qtype == 13:
            d, dmin, sc, mn, q = np_q5k.codes(raw.reshape(-1), ROWS, k)
            w = (d.astype(np.float64)[..., None] * np.repeat(sc, 32, -1) * q
                 - dmin.astype(np.float64)[..., None] * np.repeat(mn, 32, -1)).reshape(ROWS, k)
        else:
            w = np_ref.dequant(qtype, raw.reshape(-1), ROWS, k)
        if qtype == 30:  # S_abs is sum |w a| itself
            dot = w @ _dequant_act(qtype, x)
        else:
            dot = _block_dots(qtype, w, x).sum(1)
        assert np.all(np.abs(dot - y) <= 1e-12 * s_abs + 1e-300), (case, act, k)


@pytest.mark.parametrize("qtype", rd.TYPES)
def test_model_inside_bound_everywhere(qtype):
    """The unmutated model, float32 in the sequential order, is finite (no float32 term
    overflows) and inside the bound on every combination; a zero activation gives exactly 0."""
    worst = (0.0, None)
    for case, act, k in _combos(qtype):
        f, _ = rd.weight_case(qtype, case, ROWS, k)
        x = rd.act_case(act, k, rd.act_blk(qtype))
        y, s_abs, maxw, maxa = rd.reference(qtype, f, x, k)
        got = rd.model(qtype, f, x, k)
        assert np.all(np.isfinite(got)) and np.abs(got).max() < 2.0 ** 100, (case, act, k)
        b = rd.bound(qtype, k, s_abs, maxw, maxa)
        err = np.abs(got.astype(np.float64) - y)
        assert np.all(err <= b), (case, act, k, float((err / np.maximum(b, 1e-300)).max()))
        if act == "zero":
            assert not got.any()
        ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
        worst = max(worst, (ratio, (case, act, k)), key=lambda t: t[0])
    print(f"type {qtype}: worst err / bound {worst[0]:.3g} at {worst[1]}")


def _exceeds(qtype, f, x, k, mutant):
    y, s_abs, maxw, maxa = rd.reference(qtype, f, x, k)
    got = rd.model(qtype, f, x, k, mutant).astype(np.float64)
    b = rd.bound(qtype, k, s_abs, maxw, maxa)
    return bool(np.any(~np.isfinite(got) | (np.abs(got - y) > b)))


@pytest.mark.parametrize("mutant", sorted(rd.MUTANTS))
def test_mutants_exceed_the_bound(mutant):
    """Teeth: each wrong kernel leaves the bound on at least one (case, activation) for every
    type it applies to (at the widths with clamped lanes, which past_k_not_zeroed needs)."""
    for qtype in rd.MUTANTS[mutant]:
        ks = (768, 2304) if qtype in rd.KQUANTS else (576, 2080)
        caught = []
        for case, act, k in itertools.product(rd.WEIGHT_CASES, rd.ACT_CASES, ks):
            f, _ = rd.weight_case(qtype, case, ROWS, k)
            if _exceeds(qtype, f, rd.act_case(act, k, rd.act_blk(qtype)), k, mutant):
                caught.append((case, act, k))
        print(f"{mutant}, type {qtype}: caught by {len(caught)} combinations, first {caught[:3]}")
        assert caught, (mutant, qtype)


@pytest.mark.parametrize("qtype", (8, 12, 13, 14))
def test_the_gap_on_the_present_recipe(qtype):
    """The reason the new cases exist: on the data every other test feeds these paths (N(0, 0.05)
    weights through the host quantizer, the `outlier` activation) a kernel whose scale multiply
    kept 16 bits of the packed dot (mul16) stays inside the bound on Q5_K and Q6_K: it would pass
    the whole suite. (Q4_K's 16-product dot cannot pass 16 * 15 * 127 = 30480 < 2^15, so there
    the mutant is no error at all.) FINDING: the same does NOT hold for sum16. The 8-lane sum of
    the SCALED dots of a K-quant superblock, and a Q8_0 block's 32-product dot, pass 2^15 on
    this data already, so a sum kept in 16 bits the old recipe does catch. Both are asserted."""
    m = _lib()
    rng = np.random.default_rng(qtype)
    rows = 16
    inside = {}
    for k in rd.WIDTHS[qtype][1:3]:
        w = (rng.standard_normal((rows, k)) * 0.05).astype(np.float32)
        if m is not None:
            raw = m.quantize_rows(qtype, w)
        else:  # the encoder on rounded Gaussians
            f, raw = rd.weight_case(qtype, "scales_only", rows, k)
            step = 0.05 * 4 / rd._qmax(qtype)
            off = 0 if qtype == 8 else (32 if qtype == 14 else (rd._qmax(qtype) + 1) // 2)
            f["q"][:] = np.clip(np.rint(w / step).reshape(f["q"].shape) + off, -127 if qtype == 8 else 0, rd._qmax(qtype))
            raw = rd.encode(qtype, f)
        f = rd.decode_fields(qtype, raw, rows, k)
        x = rd.act_case("outlier", k, rd.act_blk(qtype))
        for mutant in ("mul16", "sum16"):
            if qtype in rd.MUTANTS[mutant]:
                inside.setdefault(mutant, []).append(not _exceeds(qtype, f, x, k, mutant))
    print(f"type {qtype}: inside the bound on the present recipe: {inside}")
    if "mul16" in inside:
        assert all(inside["mul16"])
    if m is not None:  # the finding is about the host quantizer's codes
        assert not any(inside["sum16"])
