"""TEST INFRASTRUCTURE — Q3_K (ggml type 11) restated in numpy from the public block spec.

Independent of csrc/host/quant.cpp: a packer, the dequantizer in ggml's float32 expression
order, and a `Mat` that tests swap into np_ref (monkeypatch.setattr(np_ref, "Mat", np_q3k.Mat))
so np_ref.DecodeStep reads Q3_K_S / Q3_K_M / Q3_K_L files (which also hold types 12, 13 and 14).

Block of 256 weights, 110 bytes: u8 hmask[32] | u8 qs[64] | u8 scales[12] | f16 d.
  * scale of sub-block j = e // 16: low4 = (scales[j % 8] >> 4 (j // 8)) & 0xF, high2 =
    (scales[8 + j % 4] >> 2 (j // 4)) & 3, s_j = low4 | high2 << 4, used as s_j - 32 in [-32, 31];
  * weight e: code = (qs[32 (e // 128) + e % 32] >> 2 ((e // 32) % 4)) & 3, high = (hmask[e % 32]
    >> (e // 32)) & 1, q = code + 4 high - 4 in [-4, 3];
  * value: dl = d * (s_j - 32), w = dl * q, each step rounded to float32;
  * vec_dot_type Q8_K: per superblock (d * d_a) * sum_j (s_j - 32) (q_j . a_j) with exact integer
    sums, which equals dot(dequant(w), dequant(a)) up to the float rounding of the terms, so
    `Mat @ x` is the float64 product with np_ref.act_q8_k(x).
"""
from __future__ import annotations

import numpy as np

import np_q5k
import np_ref

QTYPE = 11
BLOCK_BYTES = 110


def pack_block(d: float, s, q) -> np.ndarray:
    """One 110-byte block from an f16-representable d, 16 six-bit scales s_j (0..63; the scale
    used is s_j - 32) and 256 signed codes q in [-4, 3]."""
    s, q = np.asarray(s, np.int64), np.asarray(q, np.int64)
    assert s.shape == (16,) and s.min() >= 0 and s.max() < 64
    assert q.shape == (256,) and q.min() >= -4 and q.max() <= 3
    hmask, qs, sc = np.zeros(32, np.int64), np.zeros(64, np.int64), np.zeros(12, np.int64)
    for j in range(16):
        sc[j % 8] |= (s[j] & 0xF) << (4 * (j // 8))
        sc[8 + j % 4] |= (s[j] >> 4) << (2 * (j // 4))
    for e in range(256):
        u = int(q[e]) + 4
        qs[32 * (e // 128) + e % 32] |= (u & 3) << (2 * ((e // 32) % 4))
        hmask[e % 32] |= (u >> 2) << (e // 32)
    out = np.zeros(BLOCK_BYTES, np.uint8)
    out[0:32] = hmask.astype(np.uint8)
    out[32:96] = qs.astype(np.uint8)
    out[96:108] = sc.astype(np.uint8)
    out[108:110] = np.array([d], np.float16).view(np.uint8)
    return out


def codes(raw: np.ndarray, rows: int, k: int):
    """(d [rows, nb] f32; s [rows, nb, 16] int six-bit scales 0..63; q [rows, nb, 256] int codes in
    [-4, 3])."""
    b = np.asarray(raw, np.uint8).reshape(rows, k // 256, BLOCK_BYTES)
    hmask = b[:, :, 0:32].astype(np.int64)
    qs = b[:, :, 32:96].astype(np.int64)
    sc = b[:, :, 96:108].astype(np.int64)
    d = b[:, :, 108:110].copy().view(np.float16).astype(np.float32).reshape(rows, -1)
    s = np.zeros(sc.shape[:2] + (16,), np.int64)
    for j in range(16):
        s[..., j] = ((sc[..., j % 8] >> (4 * (j // 8))) & 0xF) | (((sc[..., 8 + j % 4] >> (2 * (j // 4))) & 3) << 4)
    q = np.zeros(sc.shape[:2] + (256,), np.int64)
    for g in range(8):  # 32 weights 32 g .. 32 g + 31
        code = (qs[..., 32 * (g // 4):32 * (g // 4) + 32] >> (2 * (g % 4))) & 3
        q[..., 32 * g:32 * g + 32] = code + 4 * ((hmask >> g) & 1) - 4
    return d, s, q


def dequant(qtype: int, raw: np.ndarray, rows: int, k: int) -> np.ndarray:
    """np_ref.dequant with type 11: float32 [rows, k] in dequantize_row_q3_K's expression order (dl =
    d * (s - 32); y = dl * q, both float32); other types: np_q5k's (13: float32, else np_ref's)."""
    if qtype != QTYPE:
        return np_q5k.dequant(qtype, raw, rows, k)
    d, s, q = codes(raw, rows, k)
    dl = (d[..., None] * (s - 32).astype(np.float32)).astype(np.float32)  # [rows, nb, 16]
    return (np.repeat(dl, 16, axis=-1) * q.astype(np.float32)).astype(np.float32).reshape(rows, k)


class Mat(np_q5k.Mat):
    """np_q5k.Mat that also reads Q3_K tensors (activation: Q8_K, as for every K-quant)."""

    def __init__(self, t):
        self.type, self.k, self.rows = t.type, t.ne[0], t.ne[1] if len(t.ne) > 1 else 1
        self.w = dequant(t.type, t.raw(), self.rows, self.k).astype(np.float64)

    def __matmul__(self, x: np.ndarray) -> np.ndarray:
        if self.type == QTYPE:
            return (self.w @ np_ref.act_q8_k(x)).astype(np.float32)
        return super().__matmul__(x)


def known_answer_block():
    """The known-answer block: d = 1, s_j = (5 j + 3) % 64, q[e] = (7 e + 3 (e // 16)) % 8 - 4
    -> (block bytes, expected w[e] = (s_j - 32) q[e])."""
    e = np.arange(256)
    j = e // 16
    s = (5 * np.arange(16) + 3) % 64
    q = (7 * e + 3 * j) % 8 - 4
    want = ((s[j] - 32) * q).astype(np.float32)
    return pack_block(1.0, s, q), want


def ceiling_block():
    """The ceiling block: every q = -4 and every s_j = 0 (scale -32), d = 1: against Q8_K codes that
    are all -127 every 16-group dot is 16 * 4 * 127 = 8128 and the superblock sum 16 * 32 * 8128."""
    return pack_block(1.0, np.zeros(16, np.int64), np.full(256, -4, np.int64))


def split_inverse(split: np.ndarray, off, rows: int, k: int):
    """The inverse of to_split for type 11, restated from the table at the top of csrc/host/quant.h:
    (d [rows, nb] f32, scale - 32 [rows, nb, 16] int, q [rows, nb, 256] int in [-4, 3]) read back
    from the planes q [R][K/4] | h [R][K/8] | sc [R][K/16] i8 | d [R][K/256] f16. Piece pc = 0..7 of
    a superblock sits at position P = 4 (pc & 1) + (pc >> 1) of each plane and holds run t = 0, 1:
    elements 64 (pc >> 1) + 16 (pc & 1) + 32 t + i, i < 16; element i's code is byte i % 4 of dword
    t of the piece's 8 q bytes at bits 2 (i // 4), its high bit is bit 4 t + i // 4 of byte i % 4
    of the piece's 4 h bytes; the run's int8 scale is byte t of the piece's 2 sc bytes."""
    nb = k // 256
    split = np.asarray(split, np.uint8)
    qp = split[off[0]:off[0] + rows * k // 4].reshape(rows, nb, 64).astype(np.int64)
    hp = split[off[1]:off[1] + rows * k // 8].reshape(rows, nb, 32).astype(np.int64)
    sp = split[off[2]:off[2] + rows * k // 16].copy().view(np.int8).reshape(rows, nb, 16).astype(np.int64)
    d = split[off[3]:off[3] + rows * nb * 2].copy().view(np.float16).astype(np.float32).reshape(rows, nb)
    sc = np.zeros((rows, nb, 16), np.int64)
    q = np.zeros((rows, nb, 256), np.int64)
    for pc in range(8):
        P = 4 * (pc & 1) + (pc >> 1)
        for t in range(2):
            e0 = 64 * (pc >> 1) + 16 * (pc & 1) + 32 * t
            sc[..., e0 // 16] = sp[..., 2 * P + t]
            for i in range(16):
                code = (qp[..., 8 * P + 4 * t + i % 4] >> (2 * (i // 4))) & 3
                high = (hp[..., 4 * P + i % 4] >> (4 * t + i // 4)) & 1
                q[..., e0 + i] = code + 4 * high - 4
    return d, sc, q
