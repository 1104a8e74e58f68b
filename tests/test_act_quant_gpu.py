"""GPU: the decode prologue's activation quantizer (llm_device.h quant_regs, run by one workgroup
through mio_hip_debug_act_quant) writes, bit for bit, the record of the numpy restatement
(np_act_quant.py), on both load paths (plain and sc1) and behind the RMSNorm; and the matvec
engine's once-per-wave row epilogues return the multi-token engine's values bit for bit."""
import numpy as np
import pytest

import miotts_amd as m
import np_act_quant as aq

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check_q8_k(device, x, w, sc1, tag):
    k = x.shape[0]
    qs, d, bs = m.debug_act_quant(device, 12, x, w, 1e-6, sc1)
    rq, rd, rb = aq.q8_k(x if w is None else aq.rms_norm(x, w, 1e-6))
    assert np.array_equal(qs[:k], rq), (tag, "codes", int((qs[:k] != rq).sum()))
    assert np.array_equal(bs[:k // 16], rb), (tag, "bsums")
    assert np.array_equal(_bits(d[:k // 256]), _bits(rd)), (tag, "d", d[:k // 256], rd)


# superblocks 1, 3, 8, 9, 24: idle waves, a partly filled pass, full, a wave with two, with three
@pytest.mark.parametrize("k", [256, 768, 2048, 2304, 6144])
def test_q8_k_record_bits(device, k):
    for name, x in aq.inputs(k).items():
        for sc1 in (False, True):
            _check_q8_k(device, x, None, sc1, (name, sc1))
    rng = np.random.default_rng(k)
    w = (1 + 0.1 * rng.standard_normal(k)).astype(np.float32)
    for name in ("random", "tie_groups_neg_first", "zero_block", "single", "half_max+127"):
        _check_q8_k(device, aq.inputs(k)[name], w, False, (name, "rmsnorm"))


@pytest.mark.parametrize("k", [768, 6144])
def test_q8_k_non_finite_inputs(device, k):
    """NaNs never are the maximum and quantize to 0; an infinite maximum gives zero codes and an
    infinite d (the quantizer's docstring)."""
    for name, x in aq.nonfinite_inputs(k).items():
        _check_q8_k(device, x, None, False, name)


@pytest.mark.parametrize("k", [576, 2048])
def test_q8_0_and_bf16_record_bits(device, k):
    rng = np.random.default_rng(k)
    w = (1 + 0.1 * rng.standard_normal(k)).astype(np.float32)
    for name, x in aq.inputs(k, 32).items():
        for wv, sc1 in ((None, False), (None, True), (w, False)):
            if wv is not None and name in ("subnormal_max", "huge_1e30"):
                continue  # squares under- / overflow: the norm is not what these inputs are for
            y = x if wv is None else aq.rms_norm(x, wv, 1e-6)
            qs, d, _ = m.debug_act_quant(device, 8, x, wv, 1e-6, sc1)
            rq, rd = aq.q8_0(y)
            assert np.array_equal(qs[:k], rq), (name, sc1, "q8_0 codes")
            assert np.array_equal(_bits(d[:k // 32]), _bits(rd)), (name, sc1, "q8_0 d")
            qs, _, _ = m.debug_act_quant(device, 30, x, wv, 1e-6, sc1)
            assert np.array_equal(qs.view(np.uint16)[:k], aq.bf16(y)), (name, sc1, "bf16")


# rows 1, 7, 9: waves own 0 or 1 rows; 17: 1 or 2; 24: 1; 6144 (added): 3 rows per wave on every
# wave of a 256-workgroup grid - the matvec grid gives a wave a third row only past 4096 rows
@pytest.mark.parametrize("qtype,rows", [(t, r) for t in (12, 14) for r in (1, 7, 9, 17, 24)] + [(12, 6144)])
def test_row_epilogues_equal_mmq(device, qtype, rows):
    """mio_hip_debug_matvec (rows parked per lane, one store per wave) against mio_hip_debug_mmq,
    bit for bit: mode 0 (store) and mode 2 (SwiGLU: the matvec side is the gate|up stream of row
    pairs with its per-lane epilogue)."""
    k = 2048
    rng = np.random.default_rng(qtype * 100 + rows)
    wq = m.quantize_rows(qtype, (rng.standard_normal((rows, k)) * 0.05).astype(np.float32))
    wu = m.quantize_rows(qtype, (rng.standard_normal((rows, k)) * 0.05).astype(np.float32))
    x = rng.standard_normal((1, k)).astype(np.float32)
    y = m.debug_matvec(device, qtype, wq, k, x[0])
    assert np.array_equal(_bits(y), _bits(m.debug_mmq(device, qtype, wq, k, x)[0]))
    g = m.debug_matvec_swiglu(device, qtype, wq, wu, k, x[0])
    assert np.array_equal(_bits(g), _bits(m.debug_mmq(device, qtype, wq, k, x, mode=2, up_rows=wu)[0]))
