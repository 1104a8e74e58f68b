"""CPU: Q5_K (ggml type 13) on the host: the block format against an independent numpy
restatement (tests/np_q5k.py), the synthetic quantizer, and Q5_K_M / Q5_K_S GGUF files."""
import numpy as np
import pytest

import miotts_amd as m
import np_q5k
import np_ref
from miotts_amd import gguf_np


def test_known_answer_block():
    """One hand-built block (d = 1, dmin = 0.5, sc_j = 8j + 5, m_j = 63 - 8j, q[e] = (7e + 5 (e // 32)
    + 3) % 32): w[e] = sc_j q[e] - 0.5 m_j exactly. The fifth-bit plane holds 16 distinct byte
    values, so a wrong bit-to-sub-block mapping cannot reproduce it."""
    blk, want = np_q5k.known_answer_block()
    assert float(want.astype(np.float64).sum()) == 126464.0
    assert want[0] == -16.5 and want[37] == 115.5 and want[255] == 1887.5
    assert len(set(blk[16:48].tolist())) == 16
    got_np = np_q5k.dequant(13, blk, 1, 256)
    assert got_np.dtype == np.float32 and np.array_equal(got_np[0], want)
    got_c = m.dequantize_rows(13, blk.reshape(1, -1), 256)
    assert np.array_equal(got_c[0], want)


def _rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def test_quantize_dequantize_rows():
    rng = np.random.default_rng(13)
    w = (rng.standard_normal((37, 2048)) * 0.02).astype(np.float32)
    wq = m.quantize_rows(13, w)
    assert wq.shape == (37, 2048 // 256 * 176)
    d_np = np_q5k.dequant(13, wq, 37, 2048)
    d_c = m.dequantize_rows(13, wq, 2048)
    assert np.array_equal(d_np.view(np.uint32), d_c.view(np.uint32))
    q = np_q5k.codes(wq, 37, 2048)[4]
    assert set(np.unique(q).tolist()) == set(range(32))
    e5 = _rel_rms(d_c, w)
    e4 = _rel_rms(m.dequantize_rows(12, m.quantize_rows(12, w), 2048), w)
    print(f"relative RMS error: Q5_K {e5:.4f}, Q4_K {e4:.4f}")
    assert e5 < e4


# the llama-quantize recipes: Q5_K_M = Q5_K everywhere, Q6_K for attn_v / ffn_down on the
# use_more_bits layers (layer 2 of preset 13's three) and the tied embedding; Q5_K_S = Q5_K
# everywhere (token_embd included), Q6_K output
def _expected_type(preset, name):
    if name.endswith("norm.weight"):
        return 0
    if preset == 13:
        if name == "token_embd.weight":
            return 14
        more = name.startswith("blk.2.") and (name.endswith("attn_v.weight") or name.endswith("ffn_down.weight"))
        return 14 if more else 13
    return 14 if name == "output.weight" else 13


@pytest.mark.parametrize("preset,file_type", [(13, 17), (14, 16)])
def test_gguf_round_trip(tmp_path, monkeypatch, preset, file_type):
    path = m.synth_llm(str(tmp_path / "q5.gguf"), preset, 1)
    g = gguf_np.GGUFReader(path)
    assert g.kv["general.file_type"] == file_type
    names = [t.name for t in g.tensors]
    assert ("output.weight" in names) == (preset == 14)
    for t in g.tensors:
        assert t.type == _expected_type(preset, t.name), (t.name, t.type)
    types = {t.type for t in g.tensors}
    assert types == {0, 13, 14}
    monkeypatch.setattr(np_ref, "Mat", np_q5k.Mat)
    ref = np_ref.DecodeStep(path, 16)
    rng = np.random.default_rng(preset)
    for pos in range(8):
        lg = ref.eval(int(rng.integers(0, 13312)), pos)
        assert lg.shape == (13312,) and np.isfinite(lg).all()


def test_presets_end_at_18(tmp_path):
    """17 and 18 are the tiny models with the 1.7B and 2.6B head shapes; nothing follows them."""
    for preset, shape in ((17, (4, 2, 128)), (18, (8, 2, 64))):
        g = gguf_np.GGUFReader(m.synth_llm(str(tmp_path / f"p{preset}.gguf"), preset, 1))
        a = g.kv["general.architecture"]
        assert (g.kv[f"{a}.attention.head_count"], g.kv[f"{a}.attention.head_count_kv"],
                g.kv[f"{a}.attention.key_length"]) == shape
    with pytest.raises(m.HipError, match="bad args"):
        m.synth_llm(str(tmp_path / "x.gguf"), 19, 1)
