"""TEST INFRASTRUCTURE (numpy only) - the weight side of the quantized row dot: block encoders
from fields, hand-built weight and activation cases at the integer ceilings, an exact reference
with a derived bound, and a model of the kernels' per-lane integer path with mutants.

What it restates: y[row] = W[row] . x on the decode step's row stream (csrc/hip/llm_device.h
lane_terms / sb_term / dot_frag / pair_term / row_total), which the int8-MFMA matmul
(llm_mmq.hip) and the prefill streams (llm_prefill.hip stream_rows_b*) reproduce bit for bit.

Types: 8 Q8_0, 12 Q4_K, 13 Q5_K, 14 Q6_K, 30 BF16 (2 Q4_0 and 6 Q5_0 run as the Q8_0 rows they
equal). Encoders are written from the public ggml block layout; the Q5_K one is vectorised and
pinned to np_q5k.pack_block in test_rowdot_ref.py. `fields` is a dict of arrays per row and
(super)block: d, dmin float16 [R, nb]; sc, mn [R, nb, 8] (Q6_K: sc int8 values [R, nb, 16]); q
[R, nb, 256 | 32] codes in ROW ORDER (element e of the block), unsigned for the K-quants (Q6_K
0..63, the -32 is the kernel's), signed for Q8_0; BF16: bits uint16 [R, k].

Excluded: a non-finite d / dmin (and a non-finite BF16 weight). Nothing else is: negative d and
dmin, -0.0, f16 subnormals, 65504, scales of -128, codes of -128, all-zero blocks are all here.
For BF16 the random bit patterns keep |w| < 2^17 so that no float32 product overflows.

REFERENCE. The activation is quantized by np_act_quant (pinned bit for bit to the GPU). Per
superblock (Q8_0: per 32-block) the integer sums isum (and imin against the bsums for Q4_K /
Q5_K) are exact int64; A = d_w d_a isum, B = dmin_w d_a imin in float64; y_ref = sum (A - B),
S_abs = sum (|A| + |B|). BF16: the exact float64 dot of the bf16 operands and sum |w x|.

BOUND, counted from llm_device.h as it stands (u = 2^-24, every operation rounds once, contraction
is off in these translation units but the subtraction is counted as rounded either way):
  * sb_term, Q4_K / Q5_K: h2f exact; d = d_w * d_a (1), (float)isum (1), d * isum (1) -> 3 u |A|;
    the same three on B; v - dmin * imin (1 on |A| + |B|): T = 4.
  * sb_term, Q6_K: d_w * d_a, (float)isum, their product: T = 3 (no min term, no subtraction).
  * dot_frag, Q8_0: (float)s is exact (|s| <= 32 * 128 * 127 < 2^24); h2f(d_w) * d_a (1) and the
    product (1): T = 2.
  * row total: `acc += dot_frag` once per pass starting from 0.0f, so n_pass - 1 rounded in-lane
    adds (n_pass = 1 for k <= 2048, 3 for k <= 6144, else 6: pick_np); then sum_lanes7's 3 levels
    (rows_joint: ror8_add, swapadd16, swapadd32 - 3 levels too); Q8_0 goes through sum8_f's 3
    levels first. Each level costs at most u * sum |terms|. D = n_pass + 2 for the K-quants and
    n_pass + 5 for Q8_0.
  bound = 2 (T + D) u S_abs + k 2^-126 max|w| max|a|. The factor 2 is the margin for higher-order
  terms and the summation order; the last term is the floor for products or sums in the float32
  subnormal range, where the hardware may flush. BF16: (k / 64 + 8) u sum |w x|
  (test_llm_gpu.py test_bf16_matvec_derived_bound's count: k / 64 sequential v_dot2 terms per
  lane, the 6-level tree, the pass sums) plus the same floor.
The constants come from this count, not from what a GPU returns.

MODEL. `model(qtype, fields, x, k, mutant)` restates the per-lane integer path - the sub-block
dots of a lane's 32 weights, the scale multiply, the 8-lane sum, the float term in float32 in
sb_term's order - and sums the terms in float32 sequentially (lane after lane, a lane's passes
first), a worse order than the kernels' trees. The mutants are deliberately wrong kernels; the
reference test shows that the cases below tell each from the reference.
"""
from __future__ import annotations

import numpy as np

import np_act_quant as aq

U = 2.0 ** -24
TYPES = (8, 12, 13, 14, 30)
KQUANTS = (12, 13, 14)
BLOCK = {8: (32, 34), 12: (256, 144), 13: (256, 176), 14: (256, 210), 30: (1, 2), 2: (32, 18), 6: (32, 22)}
WIDTHS = {8: (32, 576, 2048, 2080), 30: (32, 576, 2048, 2080), 12: (256, 768, 2048, 2304, 6144),
          13: (256, 768, 2048, 2304, 6144), 14: (256, 768, 2048, 2304, 6144)}
WEIGHT_CASES = ("ceiling", "mins_only", "scales_only", "one_field", "random_bytes", "d_extremes", "last_block")
ACT_CASES = ("const_pos", "const_neg", "alternating", "ramp", "one_hot", "zero", "zero_block", "outlier")
D_EXTREMES = (65504.0, 2.0 ** -14, 2.0 ** -24, -0.0, 0.0)

# name -> the types it applies to. mul16 leaves Q4_K out: a lane's 16-product dot is at most
# 16 * 15 * 127 = 30480 < 2^15 there, so 16 bits of it are all of it.
MUTANTS = {
    "mul16": (13, 14),
    "sum16": (8, 12, 13, 14),
    "scale_unsigned": (14,),
    "code_m128_as_p128": (8,),
    "hi_scale_bits_dropped": (12, 13),
    "min_hi_bits_dropped": (12, 13),
    "d_sign_dropped": (8, 12, 13, 14),
    "dmin_sign_dropped": (12, 13),
    "isum_via_f16": (8, 12, 13, 14),
    "q6_offset_from_wrong_bsum": (14,),
    "past_k_not_zeroed": (8, 12, 13, 14, 30),
}


def n_pass(k: int) -> int:
    """pick_np (llm_kernels.hip): passes of 2048 weights a wave makes over a row."""
    return 1 if k <= 2048 else (3 if k <= 6144 else 6)


# ---------------------------------------------------------------------------- encoders
def _f16_bytes(d) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(d, np.float16)).view(np.uint8).reshape(np.shape(d) + (2,))


def pack_scales(sc: np.ndarray, mn: np.ndarray) -> np.ndarray:
    """[.., 8] six-bit scales and mins -> [.., 12] bytes (the inverse of ggml get_scale_min_k4)."""
    sc, mn = np.asarray(sc, np.int64), np.asarray(mn, np.int64)
    assert sc.min() >= 0 and mn.min() >= 0 and sc.max() < 64 and mn.max() < 64
    s = np.zeros(sc.shape[:-1] + (12,), np.int64)
    s[..., 0:4] = sc[..., 0:4] | ((sc[..., 4:8] >> 4) << 6)
    s[..., 4:8] = mn[..., 0:4] | ((mn[..., 4:8] >> 4) << 6)
    s[..., 8:12] = (sc[..., 4:8] & 0xF) | ((mn[..., 4:8] & 0xF) << 4)
    return s.astype(np.uint8)


def unpack_scales(s: np.ndarray):
    s = np.asarray(s, np.int64)
    sc, mn = np.zeros(s.shape[:-1] + (8,), np.int64), np.zeros(s.shape[:-1] + (8,), np.int64)
    sc[..., 0:4], mn[..., 0:4] = s[..., 0:4] & 63, s[..., 4:8] & 63
    sc[..., 4:8] = (s[..., 8:12] & 0xF) | ((s[..., 0:4] >> 6) << 4)
    mn[..., 4:8] = (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)
    return sc, mn


def encode(qtype: int, f: dict) -> np.ndarray:
    """fields -> GGUF row bytes uint8 [R, row_bytes]."""
    if qtype == 30:
        return np.ascontiguousarray(f["bits"], dtype=np.uint16).view(np.uint8).reshape(f["bits"].shape[0], -1)
    q = np.asarray(f["q"], np.int64)
    R, nb = q.shape[:2]
    out = np.zeros((R, nb, BLOCK[qtype][1]), np.uint8)
    if qtype == 8:
        assert q.min() >= -128 and q.max() <= 127
        out[..., 0:2] = _f16_bytes(f["d"])
        out[..., 2:] = (q & 0xFF).astype(np.uint8)
    elif qtype in (12, 13):
        assert q.min() >= 0 and q.max() < (16 if qtype == 12 else 32)
        out[..., 0:2], out[..., 2:4] = _f16_bytes(f["d"]), _f16_bytes(f["dmin"])
        out[..., 4:16] = pack_scales(f["sc"], f["mn"])
        c = q.reshape(R, nb, 4, 2, 32)  # chunk of 64: low nibbles sub-block 2c, high 2c + 1
        nib = (c[..., 0, :] & 0xF) | ((c[..., 1, :] & 0xF) << 4)
        if qtype == 12:
            out[..., 16:144] = nib.reshape(R, nb, 128).astype(np.uint8)
        else:
            fifth = (q.reshape(R, nb, 8, 32) >> 4) << np.arange(8).reshape(8, 1)  # bit j of qh[l]
            out[..., 16:48] = fifth.sum(2).astype(np.uint8)
            out[..., 48:176] = nib.reshape(R, nb, 128).astype(np.uint8)
    elif qtype == 14:
        assert q.min() >= 0 and q.max() < 64
        sc = np.asarray(f["sc"], np.int64)
        assert sc.min() >= -128 and sc.max() <= 127
        h = q.reshape(R, nb, 2, 4, 32)  # half of 128: q1..q4 of 32 each
        lo, hi = h & 0xF, h >> 4
        ql = np.stack([lo[..., 0, :] | (lo[..., 2, :] << 4), lo[..., 1, :] | (lo[..., 3, :] << 4)], axis=3)
        qh = hi[..., 0, :] | (hi[..., 1, :] << 2) | (hi[..., 2, :] << 4) | (hi[..., 3, :] << 6)
        out[..., 0:128] = ql.reshape(R, nb, 128).astype(np.uint8)
        out[..., 128:192] = qh.reshape(R, nb, 64).astype(np.uint8)
        out[..., 192:208] = (sc & 0xFF).astype(np.uint8)
        out[..., 208:210] = _f16_bytes(f["d"])
    else:
        raise ValueError(qtype)
    return out.reshape(R, -1)


def decode_fields(qtype: int, raw: np.ndarray, rows: int, k: int) -> dict:
    """GGUF row bytes -> fields (this module's own reading of the layout; np_ref.dequant is the
    independent one the tests compare with). Types 2 / 6 come back as the Q8_0 fields they equal."""
    raw = np.asarray(raw, np.uint8)
    if qtype == 30:
        return {"bits": raw.reshape(rows, -1).view(np.uint16).reshape(rows, k).copy()}
    be, bb = BLOCK[qtype]
    b = raw.reshape(rows, k // be, bb)
    f16 = lambda a: np.ascontiguousarray(a).view(np.float16).reshape(rows, -1)
    i64 = lambda a: a.astype(np.int64)
    if qtype == 8:
        return {"d": f16(b[..., 0:2]), "q": i64(np.ascontiguousarray(b[..., 2:]).view(np.int8))}
    if qtype in (2, 6):
        qs = i64(b[..., bb - 16:])
        lo, hi = qs & 0xF, qs >> 4
        if qtype == 2:
            q = np.concatenate([lo, hi], axis=2) - 8
        else:
            qh = i64(np.ascontiguousarray(b[..., 2:6]).view(np.uint32))
            j = np.arange(16)
            q = np.concatenate([lo | (((qh >> j) & 1) << 4), hi | (((qh >> (j + 16)) & 1) << 4)], axis=2) - 16
        return {"d": f16(b[..., 0:2]), "q": q}
    if qtype in (12, 13):
        sc, mn = unpack_scales(b[..., 4:16])
        qs = i64(b[..., bb - 128:]).reshape(rows, -1, 4, 32)
        q = np.stack([qs & 0xF, qs >> 4], axis=3).reshape(rows, -1, 8, 32)
        if qtype == 13:
            q = q + 16 * ((i64(b[..., 16:48])[:, :, None, :] >> np.arange(8).reshape(8, 1)) & 1)
        return {"d": f16(b[..., 0:2]), "dmin": f16(b[..., 2:4]), "sc": sc, "mn": mn, "q": q.reshape(rows, -1, 256)}
    if qtype == 14:
        ql = i64(b[..., 0:128]).reshape(rows, -1, 2, 2, 32)
        qh = i64(b[..., 128:192]).reshape(rows, -1, 2, 32)
        parts = [(ql[..., 0, :] & 0xF) | ((qh & 3) << 4), (ql[..., 1, :] & 0xF) | (((qh >> 2) & 3) << 4),
                 (ql[..., 0, :] >> 4) | (((qh >> 4) & 3) << 4), (ql[..., 1, :] >> 4) | (((qh >> 6) & 3) << 4)]
        return {"d": f16(b[..., 208:210]), "sc": i64(np.ascontiguousarray(b[..., 192:208]).view(np.int8)),
                "q": np.stack(parts, axis=3).reshape(rows, -1, 256)}
    raise ValueError(qtype)


def values(qtype: int, f: dict) -> np.ndarray:
    """The dequantized weights float64 [R, k] the fields stand for (exact)."""
    if qtype == 30:
        return (f["bits"].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    q = np.asarray(f["q"], np.float64)
    R, nb = q.shape[:2]
    d = np.asarray(f["d"], np.float64)[..., None]
    if qtype in (8, 2, 6):
        return (d * q).reshape(R, -1)
    if qtype == 14:
        s = np.repeat(np.asarray(f["sc"], np.float64), 16, axis=-1)
        return (d * s * (q - 32)).reshape(R, -1)
    dm = np.asarray(f["dmin"], np.float64)[..., None]
    s, mm = np.repeat(np.asarray(f["sc"], np.float64), 32, -1), np.repeat(np.asarray(f["mn"], np.float64), 32, -1)
    return ((d * s) * q - dm * mm).reshape(R, -1)


# ---------------------------------------------------------------------------- weight cases
def _rand_f16(rng, shape) -> np.ndarray:
    """random finite f16 bit patterns of both signs (subnormals and zeros included)."""
    bits = rng.integers(0, 1 << 16, shape).astype(np.uint16)
    bits = np.where((bits & 0x7C00) == 0x7C00, bits & np.uint16(0xBFFF), bits).astype(np.uint16)
    return bits.view(np.float16)


def _mod_f16(rng, shape) -> np.ndarray:
    """moderate scales of both signs, f16-representable."""
    return (rng.standard_normal(shape) * 0.05 + np.where(rng.random(shape) < 0.5, 0.02, -0.02)).astype(np.float16)


def _qmax(qtype):
    return {8: 127, 12: 15, 13: 31, 14: 63}[qtype]


def _zeros(qtype: int, rows: int, k: int) -> dict:
    if qtype == 30:
        return {"bits": np.zeros((rows, k), np.uint16)}
    nb = k // BLOCK[qtype][0]
    f = {"d": np.zeros((rows, nb), np.float16), "q": np.zeros((rows, nb, BLOCK[qtype][0]), np.int64)}
    if qtype in (12, 13):
        f.update(dmin=np.zeros((rows, nb), np.float16), sc=np.zeros((rows, nb, 8), np.int64),
                 mn=np.zeros((rows, nb, 8), np.int64))
    if qtype == 14:
        f["sc"] = np.zeros((rows, nb, 16), np.int64)
    return f


def _bf16_bits(v) -> np.ndarray:
    return (np.asarray(v, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _rand_bf16(rng, shape) -> np.ndarray:
    """random bf16 bit patterns with |w| < 2^17 (exponent field <= 143), subnormals included."""
    bits = rng.integers(0, 1 << 16, shape).astype(np.uint16)
    e = (bits >> 7) & 0xFF
    return np.where(e > 143, bits & np.uint16(0xBFFF), bits).astype(np.uint16)


def _ceiling_row(qtype: int, f: dict, r: int, blocks, variant: int) -> None:
    """row r, blocks `blocks` at the ceiling values of variant `variant` (cycled):
    Q4_K / Q5_K: codes max, scales 63, mins 63, (d, dmin) in (1, 1), (-1, -1), (1, -1), (-1, 1);
    Q6_K: scale in (127, -128) x code in (63, 0) x d in (1, -1); Q8_0: code in (127, -128) x d in
    (1, -1). (BF16, +-65280 by row, is set in weight_case.)"""
    for b in blocks:
        if qtype in (12, 13):
            d, dm = ((1, 1), (-1, -1), (1, -1), (-1, 1))[variant % 4]
            f["d"][r, b], f["dmin"][r, b], f["sc"][r, b], f["mn"][r, b], f["q"][r, b] = d, dm, 63, 63, _qmax(qtype)
        elif qtype == 14:
            v = variant % 8
            f["d"][r, b], f["sc"][r, b], f["q"][r, b] = (1, -1)[v >> 2], (127, -128)[v & 1], (63, 0)[(v >> 1) & 1]
        else:
            v = variant % 4
            f["d"][r, b], f["q"][r, b] = (1, -1)[v >> 1], (127, -128)[v & 1]


def weight_case(qtype: int, name: str, rows: int, k: int, seed: int = 0):
    """-> (fields, GGUF row bytes [rows, row_bytes]). BF16 has no scales, mins or d: there
    `mins_only` / `scales_only` are random bit patterns, `d_extremes` draws the WEIGHTS from
    D_EXTREMES, and a "superblock" is 256 weights (32 where k < 256). Q8_0 has no mins (both are
    random codes with moderate d); Q6_K's `mins_only` is its -32 offset alone: codes 0."""
    assert name in WEIGHT_CASES and rows <= 40
    rng = np.random.default_rng([qtype, WEIGHT_CASES.index(name), rows, k, seed])
    f = _zeros(qtype, rows, k)
    be = BLOCK[qtype][0] if qtype != 30 else (256 if k % 256 == 0 else 32)
    nb = k // be
    if qtype == 30:
        bits = f["bits"]
        if name == "ceiling":
            bits[:] = np.where(np.arange(rows) % 2 == 0, _bf16_bits(65280.0), _bf16_bits(-65280.0))[:, None]
        elif name in ("mins_only", "scales_only", "random_bytes"):
            bits[:] = _rand_bf16(rng, bits.shape)
        elif name == "one_field":
            for r in range(rows):
                s = 32 * (r % (k // 32))
                bits[r, s:s + 32] = _bf16_bits((7 * np.arange(32) + 3) % 32 - 11.5)
        elif name == "d_extremes":
            bits[:] = _bf16_bits(np.array(D_EXTREMES, np.float32)[rng.integers(0, 5, bits.shape)])
            bits[:, ::7] = _bf16_bits(rng.standard_normal(bits[:, ::7].shape))
        else:  # last_block
            bits[0, :be] = _bf16_bits(65280.0)
            bits[rows - 1, k - be:] = _bf16_bits(65280.0)
        return f, encode(qtype, f)

    qm = _qmax(qtype)
    qlo = -128 if qtype == 8 else 0
    if name == "ceiling":
        for r in range(rows):
            _ceiling_row(qtype, f, r, range(nb), r)
    elif name in ("mins_only", "scales_only"):
        f["d"][:] = _mod_f16(rng, f["d"].shape)
        f["q"][:] = rng.integers(qlo, qm + 1, f["q"].shape)
        if qtype in (12, 13):
            f["dmin"][:] = _mod_f16(rng, f["d"].shape)
            if name == "mins_only":
                f["mn"][:] = 63
            else:
                f["sc"][:] = rng.integers(0, 64, f["sc"].shape)
        elif qtype == 14:
            f["sc"][:] = rng.integers(-128, 128, f["sc"].shape)
            if name == "mins_only":
                f["q"][:] = 0
    elif name == "one_field":
        for r in range(rows):
            b = (r // 8) % nb
            if qtype == 8:
                b = r % nb
                f["d"][r, b], f["q"][r, b] = 1, (7 * np.arange(32) + 3) % 255 - 127
                continue
            f["d"][r, b] = 1
            if qtype == 14:
                j = r % 16
                f["sc"][r, b, j] = 63
                f["q"][r, b, 16 * j:16 * j + 16] = (11 * np.arange(16) + 5 + j) % 64
            else:
                j = r % 8
                f["dmin"][r, b], f["sc"][r, b, j], f["mn"][r, b, j] = 0.5, 63, 37
                f["q"][r, b, 32 * j:32 * j + 32] = (7 * np.arange(32) + 3 + j) % (qm + 1)
    elif name in ("random_bytes", "d_extremes"):
        raw = rng.integers(0, 256, (rows, nb * BLOCK[qtype][1])).astype(np.uint8)
        f = decode_fields(qtype, raw, rows, k)
        if name == "random_bytes":
            f["d"] = _rand_f16(rng, f["d"].shape)
            if "dmin" in f:
                f["dmin"] = _rand_f16(rng, f["d"].shape)
        else:
            r, s = np.meshgrid(np.arange(rows), np.arange(nb), indexing="ij")
            ext = np.array(D_EXTREMES, np.float16)
            f["d"] = ext[(r + s) % 5]
            if "dmin" in f:
                f["dmin"] = ext[(r + 2 * s + 1) % 5]
    else:  # last_block
        _ceiling_row(qtype, f, 0, [0], 0)
        _ceiling_row(qtype, f, rows - 1, [nb - 1], 0)
    return f, encode(qtype, f)


def repacked_case(qtype: int, name: str, rows: int, k: int):
    """Q4_0 (2) / Q5_0 (6) rows, which the loader runs as the Q8_0 rows they equal -> (those
    Q8_0 fields, the Q4_0 / Q5_0 row bytes). ceiling: every code at its maximum (+7 / +15) with d
    = 1 on even rows, every code 0 (-8 / -16) with d = -1 on odd rows; random_bytes: every byte
    random, d a random finite f16."""
    assert qtype in (2, 6) and name in ("ceiling", "random_bytes")
    rng = np.random.default_rng([qtype, WEIGHT_CASES.index(name), rows, k])
    bb = BLOCK[qtype][1]
    raw = rng.integers(0, 256, (rows, k // 32, bb)).astype(np.uint8)
    if name == "ceiling":
        raw[0::2, :, 2:], raw[1::2, :, 2:] = 0xFF, 0
        d = np.where(np.arange(rows) % 2 == 0, 1.0, -1.0).astype(np.float16)[:, None] * np.ones(k // 32, np.float16)
    else:
        d = _rand_f16(rng, (rows, k // 32))
    raw[..., 0:2] = _f16_bytes(d)
    raw = raw.reshape(rows, -1)
    return decode_fields(qtype, raw, rows, k), raw


# ---------------------------------------------------------------------------- activation cases
def act_case(name: str, k: int, blk: int) -> np.ndarray:
    """x[k] float32, |x| <= 1e3. `blk` is the activation's quantization block (256 K-quants, 32
    Q8_0 / BF16)."""
    assert name in ACT_CASES
    rng = np.random.default_rng([ACT_CASES.index(name), k, blk])
    nb, i = k // blk, np.arange(k)
    if name in ("const_pos", "const_neg"):
        return np.full(k, 0.75 if name == "const_pos" else -0.75, np.float32)
    if name == "alternating":
        return np.where(i % 2 == 0, 1.5, -1.5).astype(np.float32)
    if name == "ramp":  # distinct inside a block, another slope per block
        return (((i % blk) - 0.39 * blk) * (1 + 0.25 * (i // blk)) * 0.5).astype(np.float32)
    if name == "one_hot":
        x = np.zeros(k, np.float32)
        x[k // 2 + 5] = 3.0
        return x
    if name == "zero":
        return np.zeros(k, np.float32)
    if name == "zero_block":
        x = (rng.standard_normal(k) * 2).astype(np.float32)
        x.reshape(nb, blk)[1 if nb > 2 else 0] = 0
        return x
    x = rng.standard_normal(k).astype(np.float32)  # outlier: the suite's recipe
    x[3] = -9.0
    return x


def act_blk(qtype: int) -> int:
    return 256 if qtype in KQUANTS else 32


# ---------------------------------------------------------------------------- reference + bound
_ACT_MEMO = {}


def _quant_act(kind: str, x: np.ndarray):
    """np_act_quant.q8_k / q8_0 / bf16 of x, remembered for the last few activations."""
    key = (kind, np.asarray(x, np.float32).tobytes())
    if key not in _ACT_MEMO:
        if len(_ACT_MEMO) > 64:
            _ACT_MEMO.clear()
        _ACT_MEMO[key] = {"q8_k": aq.q8_k, "q8_0": aq.q8_0, "bf16": aq.bf16}[kind](x)
    return _ACT_MEMO[key]


def _bf16_f64(bits) -> np.ndarray:
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def reference(qtype: int, f: dict, x: np.ndarray, k: int):
    """-> (y_ref, S_abs, max|w| per row, max|a|), float64."""
    w = values(qtype, f)
    maxw = np.abs(w).max(1)
    if qtype == 30:
        a = _bf16_f64(_quant_act("bf16", x))
        return w @ a, np.abs(w) @ np.abs(a), maxw, float(np.abs(a).max())
    R = w.shape[0]
    q = np.asarray(f["q"], np.int64)
    d = np.asarray(f["d"], np.float64)
    if qtype == 8:
        qa, da = _quant_act("q8_0", x)
        qa, da = qa.astype(np.int64).reshape(-1, 32), da.astype(np.float64)
        A = d * da * (q * qa).sum(-1)
        return A.sum(1), np.abs(A).sum(1), maxw, float((np.abs(qa).max(1) * da).max())
    qa, da, _ = _quant_act("q8_k", x)
    qa, da = qa.astype(np.int64).reshape(-1, 256), da.astype(np.float64)
    maxa = float((np.abs(qa).max(1) * np.abs(da)).max())
    if qtype == 14:
        dots = ((q - 32).reshape(R, -1, 16, 16) * qa.reshape(-1, 16, 16)).sum(-1)
        A = d * da * (np.asarray(f["sc"], np.int64) * dots).sum(-1)
        return A.sum(1), np.abs(A).sum(1), maxw, maxa
    dots = (q.reshape(R, -1, 8, 32) * qa.reshape(-1, 8, 32)).sum(-1)
    isum = (np.asarray(f["sc"], np.int64) * dots).sum(-1)
    imin = (np.asarray(f["mn"], np.int64) * qa.reshape(-1, 8, 32).sum(-1)).sum(-1)
    A, B = d * da * isum, np.asarray(f["dmin"], np.float64) * da * imin
    return (A - B).sum(1), (np.abs(A) + np.abs(B)).sum(1), maxw, maxa


TERM_OPS = {12: 4, 13: 4, 14: 3, 8: 2}


def bound(qtype: int, k: int, s_abs, maxw, maxa):
    floor = k * 2.0 ** -126 * np.asarray(maxw) * maxa
    if qtype == 30:
        return (k / 64 + 8) * U * np.asarray(s_abs) + floor
    depth = n_pass(k) + (5 if qtype == 8 else 2)
    return 2 * (TERM_OPS[qtype] + depth) * U * np.asarray(s_abs) + floor


# ---------------------------------------------------------------------------- the per-lane model
def _wrap16(v):
    return ((np.asarray(v, np.int64) + 32768) % 65536) - 32768


def _cvt(isum, mutant):
    with np.errstate(over="ignore"):
        if mutant == "isum_via_f16":
            return isum.astype(np.float16).astype(np.float32)
        return isum.astype(np.float32)


def _terms(qtype: int, f: dict, qa, da, bs, mutant):
    """float32 [R, n] terms of n (weight block, activation block) pairs: f's blocks against the
    activation blocks qa [n, blk], da [n], bs [n, 16]."""
    F32 = np.float32
    q = np.asarray(f["q"], np.int64)
    R, n = q.shape[:2]
    d = np.asarray(f["d"], F32)
    if mutant == "d_sign_dropped":
        d = np.abs(d)
    da = np.asarray(da, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if qtype == 8:
            if mutant == "code_m128_as_p128":
                q = np.where(q == -128, 128, q)
            s = (q * qa).sum(-1)
            if mutant == "sum16":
                s = _wrap16(s)
            return (_cvt(s, mutant) * (d * da).astype(F32)).astype(F32)
        if qtype == 14:
            sc = np.asarray(f["sc"], np.int64)
            if mutant == "scale_unsigned":
                sc = sc & 0xFF
            bsj = bs.astype(np.int64)  # [n, 16]
            if mutant == "q6_offset_from_wrong_bsum":  # the lane's b0 and b1 (sub-blocks j, j + 4) swapped
                bsj = bsj.reshape(n, 2, 2, 4)[:, :, ::-1, :].reshape(n, 16)
            t = (q.reshape(R, n, 16, 16) * qa.reshape(n, 16, 16)).sum(-1) - 32 * bsj
            if mutant == "mul16":
                t = _wrap16(t)
            isum = (sc * t).sum(-1)
            if mutant == "sum16":
                isum = _wrap16(isum)
            return ((d * da).astype(F32) * _cvt(isum, mutant)).astype(F32)
        # Q4_K / Q5_K: lane (jj, p) holds 16 codes of sub-block 2 jj and 16 of 2 jj + 1
        sc, mn = np.asarray(f["sc"], np.int64).copy(), np.asarray(f["mn"], np.int64).copy()
        if mutant == "hi_scale_bits_dropped":
            sc[..., 4:] &= 0xF
        if mutant == "min_hi_bits_dropped":
            mn[..., 4:] &= 0xF
        dots = (q.reshape(R, n, 4, 2, 2, 16) * qa.reshape(n, 4, 2, 2, 16)).sum(-1)  # [jj, half, p]
        if mutant == "mul16":
            dots = _wrap16(dots)
        lane_isum = (sc.reshape(R, n, 4, 2, 1) * dots).sum(3)
        lane_imin = (mn.reshape(R, n, 4, 2, 1) * bs.astype(np.int64).reshape(n, 4, 2, 2)).sum(3)
        isum, imin = lane_isum.sum((2, 3)), lane_imin.sum((2, 3))
        if mutant == "sum16":
            isum, imin = _wrap16(isum), _wrap16(imin)
        dm = np.asarray(f["dmin"], F32)
        if mutant == "dmin_sign_dropped":
            dm = np.abs(dm)
        v = ((d * da).astype(F32) * _cvt(isum, mutant)).astype(F32)
        return (v - ((dm * da).astype(F32) * _cvt(imin, mutant)).astype(F32)).astype(F32)


def _seq_sum(t: np.ndarray) -> np.ndarray:
    """float32 sum over the last axis, strictly left to right."""
    acc = np.zeros(t.shape[:-1], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(t.shape[-1]):
            acc = (acc + t[..., i]).astype(np.float32)
    return acc


def model(qtype: int, f: dict, x: np.ndarray, k: int, mutant: str = None) -> np.ndarray:
    """float32 y[R] of the kernels' path (module docstring), `mutant` one of MUTANTS or None."""
    assert mutant is None or qtype in MUTANTS[mutant], (mutant, qtype)
    NP = n_pass(k)
    if qtype == 30:
        w = (np.asarray(f["bits"], np.uint16).astype(np.uint32) << 16).view(np.float32)
        a = (_quant_act("bf16", x).astype(np.uint32) << 16).view(np.float32)
        R = w.shape[0]
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            prod = np.zeros((R, NP * 2048), np.float32)
            prod[:, :k] = w * a
            lanes = prod.reshape(R, NP, 4, 64, 8).transpose(0, 3, 1, 2, 4).reshape(R, 64, -1)
            y = _seq_sum(_seq_sum(lanes))
            if mutant == "past_k_not_zeroed":  # pieces past k: the row's last 8 weights and activations
                pos = (np.arange(NP)[:, None, None] * 2048 + 512 * np.arange(4)[None, :, None] + 8 * np.arange(64))
                y = (y + np.float32((pos >= k).sum()) * _seq_sum(prod[:, k - 8:k])).astype(np.float32)
        return y
    if qtype == 8:
        qa, da = _quant_act("q8_0", x)
        qa, bs, lanes = qa.astype(np.int64).reshape(-1, 32), None, 64
    else:
        qa, da, bs = _quant_act("q8_k", x)
        qa, bs, lanes = qa.astype(np.int64).reshape(-1, 256), bs.reshape(-1, 16), 8
    t = _terms(qtype, f, qa, da, bs, mutant)
    R, n = t.shape
    grid = np.zeros((R, NP * lanes), np.float32)
    grid[:, :n] = t
    if mutant == "past_k_not_zeroed" and n < NP * lanes:
        # clamped lanes: the row's last block against the activation's block 0
        last = {key: v[:, -1:] for key, v in f.items()}
        grid[:, n:] = _terms(qtype, last, qa[:1], da[:1], None if bs is None else bs[:1], None)
    return _seq_sum(_seq_sum(grid.reshape(R, NP, lanes).transpose(0, 2, 1)))
