"""GPU: the decode step's single-group row stream (every wave's share one register group of SU
units, the form the q|k|v, O, gate|up and down launches run; one-pass Q4_K / Q6_K groups reduce
their rows jointly, llm_device.h rows_joint) gives the bits of the streaming form that mio_hip_debug_matvec and
mio_hip_debug_matvec_swiglu run, which tests/test_decode_bits_gpu.py pins to the recorded fixture.

Types 12, 13, 14, 8, 30. K 256 and 2048 (one pass: SU 2, 3, 4, 6 plain, 2, 4, 6 as row pairs),
K 2560 and 6144 (three passes: SU 3, one row per wave). Two workgroups; row counts that leave
waves with no row and one row (5 rows), a partly filled group whose tail units are clamped
duplicates, and a full group. Row 1 is all zeros, row 2 holds the largest codes of both signs.
Every comparison is bitwise."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import miotts_amd as m  # noqa: E402
import record_decode_bits as R  # noqa: E402

pytestmark = pytest.mark.gpu

GRID = 2
MAX_ROWS = 16 * 6


def _inputs(qtype, k):
    """record_decode_bits' generator with the two special rows."""
    rng = np.random.default_rng(qtype * 100000 + k)
    wf = (rng.standard_normal((2, MAX_ROWS, k)) * 0.05).astype(np.float32)
    wf[:, 1] = 0.0
    wf[:, 2] = np.where(np.arange(k) % 3 == 0, 0.4, -0.4)
    wf[1, 2] = -wf[1, 2]
    x = rng.standard_normal(k).astype(np.float32)
    x[3] = -9.0
    return m.quantize_rows(qtype, wf[0]), m.quantize_rows(qtype, wf[1]), x


def _cases(k):
    """(su, pairs, rows): rows per wave <= su / (passes * matrices) on 2 x 8 waves."""
    if k > 2048:
        return [(3, False, 5), (3, False, 13), (3, False, 16)]
    out = []
    for su in (2, 3, 4, 6):
        out += [(su, False, 5), (su, False, 16 * su - 13), (su, False, 16 * su)]
        if su % 2 == 0:
            out += [(su, True, 5), (su, True, 8 * su - 5), (su, True, 8 * su)]
    return out


@pytest.mark.parametrize("qtype", R.QTYPES)
def test_group_stream_bits(device, qtype):
    bad = []
    for k in R.KS:
        wg, wu, x = _inputs(qtype, k)
        ref = {}
        for su, pairs, rows in _cases(k):
            if (pairs, rows) not in ref:
                ref[pairs, rows] = (m.debug_matvec_swiglu(device, qtype, wg[:rows], wu[:rows], k, x) if pairs
                                    else m.debug_matvec(device, qtype, wg[:rows], k, x)).view(np.uint32)
            got = m.debug_matvec_group(device, qtype, wg[:rows], wu[:rows] if pairs else None, k, x, su,
                                       GRID).view(np.uint32)
            if not np.array_equal(got, ref[pairs, rows]):
                bad.append((k, su, pairs, rows, np.flatnonzero(got != ref[pairs, rows])[:6].tolist()))
    assert not bad, (len(bad), bad[:6])


def test_group_share_checked(device):
    """A grid whose waves would own more than SU units is refused, not run."""
    wg, _, x = _inputs(12, 256)
    with pytest.raises(Exception):
        m.debug_matvec_group(device, 12, wg[:40], None, 256, x, 2, GRID)
