"""TEST INFRASTRUCTURE — Q5_K (ggml type 13) restated in numpy from the public block spec.

Independent of csrc/host/quant.cpp: a packer, the dequantizer in ggml's float32 expression
order, and a `Mat` that tests swap into np_ref (monkeypatch.setattr(np_ref, "Mat", np_q5k.Mat))
so np_ref.DecodeStep reads Q5_K_M / Q5_K_S files.

Block of 256 weights, 176 bytes: f16 d | f16 dmin | u8 scales[12] | u8 qh[32] | u8 qs[128].
  * scales: Q4_K's packing (get_scale_min_k4) of the 6-bit sc_j, m_j of sub-block j = 0..7;
  * weight e: sub-block j = e // 32, l = e % 32, chunk c = j // 2; low four bits = qs[32c + l]
    & 0xF (j even) or >> 4 (j odd); fifth bit = (qh[l] >> j) & 1; code q = low + 16 * fifth;
  * value: d1 = d * sc_j, m1 = dmin * m_j, w = d1 * q - m1, each step rounded to float32;
  * vec_dot_type Q8_K: per superblock (d * d_a) * sum_j sc_j (q_j . a_j) - (dmin * d_a) * sum_j
    m_j bsum_j with exact integer sums, which equals dot(dequant(w), dequant(a)) up to the float
    rounding of the terms, so `Mat @ x` is the float64 product with np_ref.act_q8_k(x).
"""
from __future__ import annotations

import numpy as np

import np_ref

QTYPE = 13
BLOCK_BYTES = 176


def pack_scales(sc: np.ndarray, mn: np.ndarray) -> np.ndarray:
    """8 six-bit scales and mins -> the 12 scale bytes (inverse of get_scale_min_k4)."""
    sc, mn = np.asarray(sc, np.int64), np.asarray(mn, np.int64)
    assert sc.shape == (8,) and mn.shape == (8,) and sc.max() < 64 and mn.max() < 64 and min(sc.min(), mn.min()) >= 0
    s = np.zeros(12, np.int64)
    for j in range(4):
        s[j] = sc[j] | ((sc[j + 4] >> 4) << 6)
        s[j + 4] = mn[j] | ((mn[j + 4] >> 4) << 6)
        s[j + 8] = (sc[j + 4] & 0xF) | ((mn[j + 4] & 0xF) << 4)
    return s.astype(np.uint8)


def pack_block(d: float, dmin: float, sc, mn, q) -> np.ndarray:
    """One 176-byte block from f16-representable d, dmin, 8 scales, 8 mins and 256 codes 0..31."""
    q = np.asarray(q, np.int64)
    assert q.shape == (256,) and q.min() >= 0 and q.max() < 32
    out = np.zeros(BLOCK_BYTES, np.uint8)
    out[0:2] = np.array([d], np.float16).view(np.uint8)
    out[2:4] = np.array([dmin], np.float16).view(np.uint8)
    out[4:16] = pack_scales(sc, mn)
    qh = np.zeros(32, np.int64)
    qs = np.zeros(128, np.int64)
    for e in range(256):
        j, l = divmod(e, 32)
        qh[l] |= (q[e] >> 4) << j
        qs[32 * (j // 2) + l] |= (q[e] & 0xF) << (4 * (j & 1))
    out[16:48] = qh.astype(np.uint8)
    out[48:176] = qs.astype(np.uint8)
    return out


def codes(raw: np.ndarray, rows: int, k: int):
    """(d, dmin [rows, nb] f32; sc, mn [rows, nb, 8] int; q [rows, nb, 256] int codes 0..31)."""
    b = np.asarray(raw, np.uint8).reshape(rows, k // 256, BLOCK_BYTES)
    d = b[:, :, 0:2].copy().view(np.float16).astype(np.float32).reshape(rows, -1)
    dmin = b[:, :, 2:4].copy().view(np.float16).astype(np.float32).reshape(rows, -1)
    s = b[:, :, 4:16].astype(np.int64)
    qh = b[:, :, 16:48].astype(np.int64)
    qs = b[:, :, 48:176].astype(np.int64)
    sc = np.zeros(s.shape[:2] + (8,), np.int64)
    mn = np.zeros_like(sc)
    for j in range(8):
        if j < 4:
            sc[..., j] = s[..., j] & 63
            mn[..., j] = s[..., j + 4] & 63
        else:
            sc[..., j] = (s[..., j + 4] & 0xF) | ((s[..., j - 4] >> 6) << 4)
            mn[..., j] = (s[..., j + 4] >> 4) | ((s[..., j] >> 6) << 4)
    q = np.zeros(s.shape[:2] + (256,), np.int64)
    for j in range(8):
        nib = qs[..., 32 * (j // 2):32 * (j // 2) + 32]
        low = (nib >> 4) if (j & 1) else (nib & 0xF)
        q[..., 32 * j:32 * j + 32] = low + 16 * ((qh >> j) & 1)
    return d, dmin, sc, mn, q


def dequant(qtype: int, raw: np.ndarray, rows: int, k: int) -> np.ndarray:
    """np_ref.dequant with type 13: float32 [rows, k] in dequantize_row_q5_K's expression order
    (d1 = d * sc; m1 = min * m; y = d1 * q - m1, all float32); other types: np_ref's float64."""
    if qtype != QTYPE:
        return np_ref.dequant(qtype, raw, rows, k)
    d, dmin, sc, mn, q = codes(raw, rows, k)
    d1 = (d[..., None] * sc.astype(np.float32)).astype(np.float32)        # [rows, nb, 8]
    m1 = (dmin[..., None] * mn.astype(np.float32)).astype(np.float32)
    prod = (np.repeat(d1, 32, axis=-1) * q.astype(np.float32)).astype(np.float32)
    return (prod - np.repeat(m1, 32, axis=-1)).astype(np.float32).reshape(rows, k)


class Mat(np_ref.Mat):
    """np_ref.Mat that also reads Q5_K tensors (activation: Q8_K, as for every K-quant)."""

    def __init__(self, t):
        self.type, self.k, self.rows = t.type, t.ne[0], t.ne[1] if len(t.ne) > 1 else 1
        self.w = dequant(t.type, t.raw(), self.rows, self.k).astype(np.float64)

    def __matmul__(self, x: np.ndarray) -> np.ndarray:
        if self.type == QTYPE:
            return (self.w @ np_ref.act_q8_k(x)).astype(np.float32)
        return super().__matmul__(x)


def known_answer_block():
    """The known-answer block of the Q5_K tests: d = 1, dmin = 0.5, sc_j = 8j + 5, m_j = 63 - 8j,
    q[e] = (7e + 5 (e // 32) + 3) % 32 -> (block bytes, expected w[e] = sc_j q[e] - 0.5 m_j)."""
    e = np.arange(256)
    j = e // 32
    sc, mn = 8 * np.arange(8) + 5, 63 - 8 * np.arange(8)
    q = (7 * e + 5 * j + 3) % 32
    want = (sc[j] * q - 0.5 * mn[j]).astype(np.float32)
    return pack_block(1.0, 0.5, sc, mn, q), want
