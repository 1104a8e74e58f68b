"""CPU: the host's Q8_0 K/V row quantizer and the dequantize-to-f16 rule (miotts_amd.kv_q8_0) against
the float64 restatement np_kv_q8.rows, bit for bit, on the blocks that decide it."""
import numpy as np
import pytest

import miotts_amd as m
import np_kv_q8

_rng = np.random.default_rng(3)
BLOCKS = {
    "zero": np.zeros(32),                                   # d = 0: id = 0, codes 0, values +0
    # amax 127: d = id = 1, so x = n + 0.5 are exact ties (away from zero: 3, -4, 1, -1, 126, -126)
    "ties": np.r_[127.0, 2.5, -3.5, 0.5, -0.5, 125.5, -125.5, np.arange(25) - 12.0],
    "pm127": np.r_[-3.0, 3.0, _rng.uniform(-3, 3, 30)],     # both signs land on +-127
    "tiny": np.r_[2.0 ** -24, -(2.0 ** -24), np.zeros(30)],  # d underflows f16: scale 0, values 0
    "random": _rng.standard_normal(32 * 64) * np.repeat(2.0 ** _rng.integers(-12, 12, 64), 32),
}


@pytest.mark.parametrize("name", BLOCKS)
def test_rows_equal_the_float64_restatement(name):
    x = BLOCKS[name].astype(np.float16).reshape(-1, 32 if name != "random" else 128)
    q, d, v = m.kv_q8_0(x)
    qr, dr, vr = np_kv_q8.rows(x)
    assert q.dtype == np.int8 and d.dtype == v.dtype == np.float16
    assert np.array_equal(q, qr) and np.array_equal(d.view(np.uint16), dr.view(np.uint16))
    assert np.array_equal(v.view(np.uint16), vr.view(np.uint16))
    if name == "ties":
        assert q.reshape(-1)[:7].tolist() == [127, 3, -4, 1, -1, 126, -126]
    if name == "pm127":
        assert q.min() == -127 and q.max() == 127
    if name == "random":  # the f16 scale rounds up in some blocks and down in others
        exact = np.abs(x.astype(np.float64).reshape(-1, 32)).max(axis=1) / 127.0
        assert (d.reshape(-1) > exact).any() and (d.reshape(-1) < exact).any()
