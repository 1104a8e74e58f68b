"""TEST INFRASTRUCTURE — IQ4_XS (ggml type 23) restated in numpy from the public block spec.

Independent of csrc/host/quant.cpp. Block of 256 weights, 136 bytes: f16 d | u16 scales_h |
u8 scales_l[4] | u8 qs[128]; sub-block ib = e // 32 has ls = ((scales_l[ib // 2] >> 4 (ib % 2)) & 0xF)
| (((scales_h >> 2 ib) & 3) << 4), dl = d * (ls - 32); its element j < 16 is dl * KV[qs[16 ib + j] & 0xF]
and element j + 16 is dl * KV[qs[16 ib + j] >> 4], each step rounded to float32. vec_dot_type Q8_K,
so `Mat @ x` is the float64 product with np_ref.act_q8_k(x), as for every K-quant.
"""
import numpy as np

import np_q5k
import np_ref

QTYPE = 23
BLOCK_BYTES = 136
KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int64)


def fields(raw, rows: int, k: int):
    """(d [rows, nb] f32, ls [rows, nb, 8] int 0..63, code [rows, nb, 256] int 0..15)."""
    b = np.asarray(raw, np.uint8).reshape(rows, k // 256, BLOCK_BYTES)
    d = b[:, :, 0:2].copy().view(np.float16).astype(np.float32).reshape(rows, -1)
    sh = b[:, :, 2].astype(np.int64) | (b[:, :, 3].astype(np.int64) << 8)
    sl, qs = b[:, :, 4:8].astype(np.int64), b[:, :, 8:136].astype(np.int64).reshape(rows, -1, 8, 16)
    ib = np.arange(8)
    ls = ((sl[..., ib // 2] >> (4 * (ib % 2))) & 0xF) | (((sh[..., None] >> (2 * ib)) & 3) << 4)
    code = np.concatenate([qs & 0xF, qs >> 4], axis=-1).reshape(rows, -1, 256)
    return d, ls, code


def dequant(raw, rows: int, k: int) -> np.ndarray:
    """float32 [rows, k] in dequantize_row_iq4_xs's order: dl = d * (ls - 32); y = dl * kv."""
    d, ls, code = fields(raw, rows, k)
    dl = (d[..., None] * (ls - 32).astype(np.float32)).astype(np.float32)
    return (np.repeat(dl, 32, axis=-1) * KV[code].astype(np.float32)).astype(np.float32).reshape(rows, k)


class Mat(np_q5k.Mat):
    """np_q5k.Mat that also reads IQ4_XS tensors."""

    def __init__(self, t):
        if t.type != QTYPE:
            return super().__init__(t)
        self.type, self.k, self.rows = t.type, t.ne[0], t.ne[1] if len(t.ne) > 1 else 1
        self.w = dequant(t.raw(), self.rows, self.k).astype(np.float64)

    def __matmul__(self, x):
        if self.type == QTYPE:
            return (self.w @ np_ref.act_q8_k(x)).astype(np.float32)
        return super().__matmul__(x)


def _pack(d: float, ls, code) -> np.ndarray:
    out = np.zeros(BLOCK_BYTES, np.uint8)
    out[0:2] = np.array([d], np.float16).view(np.uint8)
    sh = 0
    for ib in range(8):
        out[4 + ib // 2] |= (ls[ib] & 0xF) << (4 * (ib % 2))
        sh |= (ls[ib] >> 4) << (2 * ib)
        for j in range(16):
            out[8 + 16 * ib + j] = code[32 * ib + j] | (code[32 * ib + j + 16] << 4)
    out[2], out[3] = sh & 0xFF, sh >> 8
    return out


KA_LS = (0, 31, 32, 63, 17, 46, 5, 58)  # high bit pairs 0 1 2 3 | 1 2 0 3: no two of a scales_h byte alike


def known_answer_block():
    """d = 0.5, ls = KA_LS, code[e] = (e + 3 (e // 32)) % 16: every nibble value in low and in high
    position of every sub-block -> (block bytes, expected w[e] = 0.5 (ls - 32) KV[code])."""
    e = np.arange(256)
    code = (e + 3 * (e // 32)) % 16
    want = (0.5 * (np.array(KA_LS)[e // 32] - 32) * KV[code]).astype(np.float32)
    return _pack(0.5, KA_LS, code), want


def ceiling_block():
    """Every nibble 0 (kv -127), every ls 0 (scale -32), d = 1: every weight is 4064; against Q8_K codes
    that are all -127 the superblock's integer sum is -32 * 127 * 127 * 32 * 8 = -132 128 768."""
    return _pack(1.0, (0,) * 8, np.zeros(256, np.int64))
