"""CPU: mio_synth_llm_gguf_shape (a preset's rules written with sizes of the caller's; the
presets stay as numbered, tests/test_q5k_host.py::test_presets_end_at_18) and the NULL-handle
answer of mio_hip_llm_prompt_chunks."""
import ctypes
import os

import pytest

import miotts_amd as m
from miotts_amd import gguf_np


def test_shape_entry_writes_the_requested_sizes(tmp_path):
    """The lfm2 preset 7 as BF16 at the LFM2-350M width, cut to 2 layers and a small FFN here (a
    CPU test writes no 100 MB file): the sizes asked for, head_dim and the layer-kind rule of the
    preset, and with recipe 30 every matrix BF16 but the F32 conv taps."""
    g = gguf_np.GGUFReader(m.synth_llm_shape(str(tmp_path / "s.gguf"), 7, 30, 1, n_embd=1024, n_layer=2, n_head=16,
                                             n_head_kv=8, n_ff=256))
    kv = g.kv
    assert kv["general.architecture"] == "lfm2" and kv["general.file_type"] == 32
    assert (kv["lfm2.embedding_length"], kv["lfm2.block_count"], kv["lfm2.feed_forward_length"],
            kv["lfm2.attention.head_count"], kv["lfm2.attention.key_length"]) == (1024, 2, 256, 16, 64)
    assert list(kv["lfm2.attention.head_count_kv"]) == [0, 8]  # preset 7: attention at i % 3 == 1
    t = g.by_name
    assert t["blk.0.shortconv.in_proj.weight"].ne == [1024, 3072]
    assert t["blk.0.shortconv.out_proj.weight"].ne == [1024, 1024]
    assert t["blk.0.shortconv.conv.weight"].ne == [3, 1024] and t["blk.0.shortconv.conv.weight"].type == 0
    assert t["blk.1.attn_q.weight"].ne == [1024, 1024] and t["blk.1.attn_k.weight"].ne == [1024, 512]
    assert t["blk.1.ffn_down.weight"].ne == [256, 1024]
    for x in g.tensors:
        if len(x.ne) >= 2 and x.name != "blk.0.shortconv.conv.weight":
            assert x.type == 30, (x.name, x.type)
        else:
            assert x.type == 0, (x.name, x.type)


def test_zero_keeps_the_presets_sizes(tmp_path):
    a = m.synth_llm_shape(str(tmp_path / "a.gguf"), 7, 30, 1)
    b = m.synth_llm_as(str(tmp_path / "b.gguf"), 7, 30, 1)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_refusals(tmp_path):
    p = str(tmp_path / "x.gguf")
    # synth_llm_check: the Q5_K recipes need multiples of 256
    with pytest.raises(m.HipError, match="multiples of 256"):
        m.synth_llm_shape(p, 7, 17, 1, n_embd=320, n_head=5, n_head_kv=5)
    with pytest.raises(m.HipError, match="bad args"):
        m.synth_llm_shape(p, 19, 30, 1)
    with pytest.raises(m.HipError, match="unknown recipe"):
        m.synth_llm_shape(p, 7, 31, 1)
    with pytest.raises(m.HipError, match="multiples of 32"):
        m.synth_llm_shape(p, 7, 30, 1, n_embd=250)
    with pytest.raises(m.HipError, match="heads"):
        m.synth_llm_shape(p, 7, 30, 1, n_head=4, n_head_kv=3)
    with pytest.raises(m.HipError, match="bad args"):
        m.synth_llm(p, 19, 1)
    assert not os.path.exists(p)


def test_prompt_chunks_null_handle():
    L = m.lib()
    v = ctypes.c_int(-7)
    assert L.mio_hip_llm_prompt_chunks(None, ctypes.byref(v)) == -1  # MIO_ERR_INVALID
    assert b"null" in L.mio_hip_last_error() and v.value == -7
