"""CPU: the numpy restatement of the activation quantizers (np_act_quant.py) equals the oracle's
quantize_row_q8_K_ref / quantize_row_q8_0_ref on every finite, normal test input, and the test
inputs tell five wrong quantizers from it."""
import ctypes

import numpy as np
import pytest

import np_act_quant as aq
import pyoracle

# inputs on which ggml's reference is defined (its nearest_int needs |iscale * x| < 2^22)
_FINITE = [n for n in aq.inputs(256) if n != "subnormal_max"]


def _oracle_q8_k(x):
    o = pyoracle.oracle()
    k = x.shape[0]
    qs, d, bs = np.empty(k, np.int8), np.empty(k // 256, np.float32), np.empty(k // 16, np.int16)
    o.mo_quantize_q8_K.restype = None
    o.mo_quantize_q8_K.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    o.mo_quantize_q8_K(x.ctypes.data, k, d.ctypes.data, qs.ctypes.data, bs.ctypes.data)
    return qs, d, bs


def _oracle_q8_0(x):
    o = pyoracle.oracle()
    k = x.shape[0]
    qs, d = np.empty(k, np.int8), np.empty(k // 32, np.uint16)
    o.mo_quantize_q8_0.restype = None
    o.mo_quantize_q8_0.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    o.mo_quantize_q8_0(x.ctypes.data, k, d.ctypes.data, qs.ctypes.data)
    return qs, d


def _same(a, b):
    return all(np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8))
               for u, v in zip(a, b))


@pytest.mark.parametrize("k", [256, 768, 2304])
def test_q8_k_equals_the_oracle(k):
    xs = aq.inputs(k)
    for name in _FINITE:
        assert _same(aq.q8_k(xs[name]), _oracle_q8_k(xs[name])), name


@pytest.mark.parametrize("k", [576, 2048])
def test_q8_0_equals_the_oracle(k):
    xs = aq.inputs(k, 32)
    for name in _FINITE:
        qs, d = aq.q8_0(xs[name])
        oq, od = _oracle_q8_0(xs[name])
        assert np.array_equal(qs, oq) and np.array_equal(d.astype(np.float16).view(np.uint16), od), name


def test_saturating_conversion_cases():
    """What the restatement says where ggml's reference is undefined."""
    x = np.zeros(256, np.float32)
    x[0], x[1], x[2] = 1e-40, -1e-40, 5e-41  # iscale = -inf: -inf -> INT_MIN (byte 0), +inf -> 127
    qs, d, bs = aq.q8_k(x)
    assert list(qs[:4]) == [0, 127, 0, 0] and bs[0] == 127 and d[0] == 0 and np.signbit(d[0])
    x = np.ones(256, np.float32)
    x[5] = np.inf  # iscale = -0: every code 0 (inf * 0 = NaN -> 0), d = 1 / -0
    qs, d, bs = aq.q8_k(x)
    assert not qs.any() and not bs.any() and d[0] == -np.inf
    x = np.full(256, np.nan, np.float32)
    x[9] = 0.0
    qs, d, bs = aq.q8_k(x)
    assert not qs.any() and not bs.any() and d[0] == 0
    x[9] = -2.0  # NaNs beside a finite maximum: code 0, never the maximum
    qs, d, bs = aq.q8_k(x)
    assert qs[9] == -127 and qs.sum() == -127 and d[0] == np.float32(1) / (np.float32(-127) / np.float32(-2))


_CATCHES = {"last_max": "tie_groups_pos_first", "half_away": "half_max+127", "clamp_128": "subnormal_max",
            "bsums_shifted": "random", "d_from_abs": "tie_lane_neg_first"}


@pytest.mark.parametrize("mutant", aq.MUTANTS)
def test_inputs_catch_mutant(mutant):
    """last max instead of first, half-away rounding, clamp at 128, bsums over the wrong 16, d
    from |max|: each differs from the reference on the named test input, at every K the GPU test runs."""
    for k in (256, 768, 2048, 2304, 6144):
        xs = aq.inputs(k)
        assert not _same(aq.q8_k(xs[_CATCHES[mutant]], mutant), aq.q8_k(xs[_CATCHES[mutant]])), k


def test_bf16_and_roundf():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e38, np.inf, 0.0], np.float32)
    # 1 + 2^-8 ties to even (down), 1 + 3 * 2^-8 ties to even (up)
    assert list(aq.bf16(x)) == [0x3F80, 0x3F80, 0x3F82, 0xFF62, 0x7F80, 0]
    assert aq.bf16(np.array([np.nan], np.float32))[0] & 0x7FC0 == 0x7FC0
    v = np.array([0.5, -0.5, 1.5, 2.5, 0.49999997, -2.5, 8388609.0], np.float32)
    assert list(aq._roundf(v)) == [1, -1, 2, 3, 0, -3, 8388609]


def test_rms_norm_matches_float64():
    rng = np.random.default_rng(3)
    for k in (768, 2048):
        x, w = rng.standard_normal(k).astype(np.float32), rng.standard_normal(k).astype(np.float32)
        x64 = x.astype(np.float64)
        want = x64 / np.sqrt(np.mean(x64 * x64) + 1e-6) * w
        assert np.abs(aq.rms_norm(x, w, 1e-6) - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()
