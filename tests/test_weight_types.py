"""The weight-type table (csrc/weight_types.h) as the host sites read it: the split layout's plane
strides and split_layout's offsets against plane shapes restated here (and np_q3k's), qmat_rows on
every type, the (q|k, attn_v) type pairs written out, and the loader's refusal text."""
import numpy as np
import pytest

import miotts_amd as m
import np_q3k

Q8_0, Q3_K, Q4_K, Q5_K, Q6_K, BF16 = 8, 11, 12, 13, 14, 30
ROWS = 5

# The planes of one row of K weights as numpy shapes (items, dtype), restated from the layout's
# description and independent of the table: Q8_0 codes | f16 d per 32; Q3_K 2-bit codes | high
# bits | int8 scales per 16 | f16 d per 256; Q4_K nibbles | 16-B header per 256; Q5_K nibbles |
# fifth bits | header; Q6_K low nibbles | high 2 bits | int8 scales per 16 | f16 d; BF16 values.
PLANES = {
    Q8_0: lambda k: [((k,), np.int8), ((k // 32,), np.float16)],
    Q3_K: lambda k: [((k // 4,), np.uint8), ((k // 8,), np.uint8), ((k // 16,), np.int8), ((k // 256,), np.float16)],
    Q4_K: lambda k: [((k // 2,), np.uint8), ((k // 256, 16), np.uint8)],
    Q5_K: lambda k: [((k // 2,), np.uint8), ((k // 8,), np.uint8), ((k // 256, 16), np.uint8)],
    Q6_K: lambda k: [((k // 2,), np.uint8), ((k // 4,), np.uint8), ((k // 16,), np.int8), ((k // 256,), np.float16)],
    BF16: lambda k: [((k,), np.uint16)],
}
CASES = [(t, k) for t in (Q3_K, Q4_K, Q5_K, Q6_K) for k in (256, 768, 2304)] + \
        [(t, k) for t in (Q8_0, BF16) for k in (32, 96, 2304)]


def _strides(t, k):
    s = [np.zeros(shape, dt).nbytes for shape, dt in PLANES[t](k)]
    return s + [0] * (4 - len(s))


@pytest.mark.parametrize("t,k", CASES)
def test_plane_strides_and_split_layout_offsets(t, k):
    want = _strides(t, k)
    stride, off, _ = m.weight_layout(t, ROWS, k)
    assert stride == want
    # each plane starts where the planes before it end, rounded up to 256 B
    o, offs = 0, []
    for s in want:
        offs.append(o if s else 0)
        o = (o + ROWS * s + 255) // 256 * 256 if s else o
    assert off == offs
    # to_split reports the same offsets and a size that ends with the last plane
    be, bb = m.GGML_BLOCK[t]
    split, off2 = m.to_split(t, np.zeros((ROWS, k // be * bb), np.uint8), k)
    assert off2 == off and split.size == o
    if t == Q3_K:  # np_q3k.split_inverse carves its planes by its own restated sizes
        d, s, q = np_q3k.split_inverse(split, off, ROWS, k)
        assert d.shape == (ROWS, k // 256) and q.shape[:2] == (ROWS, k // 256)


@pytest.mark.parametrize("t,k", CASES)
def test_qmat_rows_moves_every_plane_by_its_stride(t, k):
    """Rows [3, 5): every plane pointer moves by 3 row strides, and by 0 where the type has no such
    plane (BF16's three, once the missing case: lfm2's X rows were read from the B rows)."""
    want = _strides(t, k)
    _, _, moved = m.weight_layout(t, ROWS, k, 3, 2)
    assert moved == [3 * s for s in want]
    assert [mv == 0 for mv in moved] == [s == 0 for s in want]


def test_attn_v_supported_is_exactly_the_eleven_pairs():
    ids = (Q8_0, Q3_K, Q4_K, Q5_K, Q6_K, BF16)
    pairs = {(8, 8), (11, 11), (11, 12), (11, 13), (12, 12), (12, 14), (13, 13), (13, 14), (14, 14), (14, 12),
             (30, 30)}
    got = {(tq, tv) for tq in ids for tv in ids if m.attn_v_supported(tq, tv)}
    assert len(ids) ** 2 == 36 and got == pairs


def test_no_layout_for_other_types():
    for t in (0, 1, 2, 6, 7, 15):  # F32, F16, Q4_0, Q5_0, Q5_1, Q8_K: not device weight types
        with pytest.raises(m.HipError):
            m.weight_layout(t, ROWS, 256)


@pytest.mark.gpu
def test_refusal_names_every_supported_type(device, synth_llm_path, tmp_path):
    """A matrix of a type the GGUF reader knows but no kernel streams (I8, declared on a Q8_0
    tensor's bytes) is refused by upload_qmat with the list of the types that are streamed."""
    from test_q5k_gpu import _retype
    dst = str(tmp_path / "i8.gguf")
    _retype(synth_llm_path(0), dst, "blk.0.ffn_up.weight", 24)
    with pytest.raises(m.HipError) as e:
        m.Llm(device, dst, 64)
    assert "blk.0.ffn_up.weight" in str(e.value) and "supported:" in str(e.value), str(e.value)
    text = str(e.value).split("supported:")[1]
    for name in ("q8_0", "q3_K", "q4_K", "q5_K", "q6_K", "bf16", "q5_0", "q4_0"):
        assert name in text, (name, text)
