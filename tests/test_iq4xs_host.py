"""CPU: IQ4_XS (ggml type 23) on the host: the dequantizer against np_iq4xs, the quantizer's round
trip within its stated error, the split layout read back by a numpy inverse and the plane strides."""
import numpy as np
import pytest

import miotts_amd as m
import np_iq4xs


def _rows(k, n=24, seed=23):
    return (0.05 * np.random.default_rng(seed + k).standard_normal((n, k))).astype(np.float32)


def test_hand_packed_blocks():
    blk, want = np_iq4xs.known_answer_block()
    assert np.array_equal(np_iq4xs.dequant(blk, 1, 256)[0], want)
    assert np.array_equal(m.dequantize_rows(23, blk.reshape(1, -1), 256)[0], want)
    assert np.array_equal(m.dequantize_rows(23, np_iq4xs.ceiling_block().reshape(1, -1), 256)[0], np.full(256, 4064.0))


@pytest.mark.parametrize("k", [256, 768, 2048])
def test_quantize_round_trip(k):
    """Each code is the nearest table entry of x / dl, and the table's widest gap is 24 (89 .. 113)
    while its ends are -127 and 113, so inside a sub-block |x - dl kv| <= 14 |dl| (the positive end);
    dl differs from the ideal amax / 127 by at most half a step of d from rounding ls (a whole step
    where ls clamps at 63) plus d's f16 rounding (2^-11 of 32 * 127 d), each times |v| <= 127: in all
    |err| <= 14 / 127 amax(sub-block) + 130 |d| per element. Over a row of N(0, sigma) weights the error is
    close to uniform within half a table gap: with the gaps' mean square (12 .. 24, about 17^2) over 12
    and a sub-block's amax near 2.1 sigma that is 17 / sqrt(12) / 127 * 2.1 = 0.08 of sigma; DESIGN.md
    states 0.080, held here to 0.085."""
    x = _rows(k)
    raw = m.quantize_rows(23, x)
    assert raw.shape == (24, k // 256 * 136)
    got = m.dequantize_rows(23, raw, k)
    assert np.array_equal(got.view(np.uint32), np_iq4xs.dequant(raw, 24, k).view(np.uint32))
    d = np_iq4xs.fields(raw, 24, k)[0]
    amax = np.abs(x.reshape(24, -1, 32)).max(-1)
    bound = np.repeat(14.0 / 127 * amax, 32, axis=-1) + np.repeat(130.0 * np.abs(d), 256, axis=-1)
    err = np.abs(got.astype(np.float64) - x)
    rms = float(np.sqrt(np.mean(err ** 2)) / np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    print(f"k {k}: relative rms error {rms:.4f}, worst err / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound) and rms <= 0.085


def _split_inverse(split, off, rows, k):
    """quant.h: qs byte 32 (e // 64) + e % 32, nibble (e // 32) % 2 | sc int8 ls - 32 | f16 d."""
    nb, e = k // 256, np.arange(256)
    qs = split[off[0]:off[0] + rows * k // 2].reshape(rows, nb, 128).astype(np.int64)
    sc = split[off[1]:off[1] + rows * nb * 8].copy().view(np.int8).reshape(rows, nb, 8).astype(np.int64)
    d = split[off[2]:off[2] + rows * nb * 2].copy().view(np.float16).astype(np.float32).reshape(rows, nb)
    return d, sc, (qs[..., 32 * (e // 64) + e % 32] >> (4 * ((e // 32) % 2))) & 0xF


def test_split_layout_round_trips():
    k = 768
    rows = np.stack([np.tile(np_iq4xs.known_answer_block()[0], 3), np.tile(np_iq4xs.ceiling_block(), 3)] +
                    list(m.quantize_rows(23, _rows(k, n=5))))
    split, off = m.to_split(23, rows, k)
    d, sc, code = _split_inverse(split, off, len(rows), k)
    d0, ls0, code0 = np_iq4xs.fields(rows, len(rows), k)
    assert np.array_equal(d, d0) and np.array_equal(sc, ls0 - 32) and np.array_equal(code, code0)


@pytest.mark.parametrize("k", [256, 2304])
def test_weight_layout_strides(k):
    want = [k // 2, k // 256 * 8, k // 256 * 2, 0]  # nibbles | 8 int8 scales | f16 d per superblock
    stride, off, moved = m.weight_layout(23, 5, k, 3, 2)
    assert stride == want and moved == [3 * s for s in want]
    up = lambda n: (n + 255) // 256 * 256  # each plane starts on the next 256 B
    assert off == [0, up(5 * want[0]), up(5 * want[0]) + up(5 * want[1]), 0]
