"""GPU: the decode step's attention launches and row streams give the bits they gave before their
serial instruction streams (the merge's weights and loads, head preparation, the row dots' header
handling) were shortened.

tests/golden/decode_bits_parent.npz was recorded on the MI355X by tools/record_decode_bits.py at
15e1913, the commit before those changes; that file describes the cases (its generators are used
here, so both sides run the same inputs): mio_hip_llm_debug_attention at the head shapes
(128, 2), (64, 3), (64, 4), launches 1 and 10, 12 positions around every 8-chunk merge batch
edge, an ordinary state and one whose chunk maxima differ by more than 100; mio_hip_debug_matvec
and mio_hip_debug_matvec_swiglu for types 12, 13, 14, 8, 30 at K 256 .. 6144, rows 1 .. 67.
Every comparison is bitwise."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import miotts_amd as m  # noqa: E402
import np_attn as A  # noqa: E402
import record_decode_bits as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(R.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _compare(golden, prefix, got):
    want = {k[len(prefix):] for k in golden if k.startswith(prefix)}
    assert want == set(got) and want, (prefix, sorted(want ^ set(got))[:8])
    bad = [k for k, v in got.items() if v.shape != golden[prefix + k].shape or not np.array_equal(v, golden[prefix + k])]
    assert not bad, (prefix, len(bad), len(got), bad[:8],
                     int((got[bad[0]] != golden[prefix + bad[0]]).sum()) if got[bad[0]].shape == golden[prefix + bad[0]].shape else -1)


@pytest.mark.parametrize("preset", R.PRESETS)
def test_attention_bits(device, synth_llm_path, golden, preset):
    path = synth_llm_path(preset)
    g, C = m.Llm(device, path, R.N_CTX), A.Cases(A.Model(path), n_ctx=R.N_CTX)
    try:
        for pattern in R.PATTERNS:
            _compare(golden, f"p{preset}_{pattern}_", R.attention_outputs(g, C, pattern))
    finally:
        g.close()


@pytest.mark.parametrize("qtype", R.QTYPES)
def test_row_dot_bits(device, golden, qtype):
    _compare(golden, f"t{qtype}_", R.matvec_outputs(device, qtype))
