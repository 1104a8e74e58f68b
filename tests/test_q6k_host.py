"""CPU: all-Q6_K GGUF files (llama-quantize's MOSTLY_Q6_K, llama_ftype 18) from the synthetic
writer's `synth_llm_as`, and the two CPU references on such a file.

The recipe: every matrix of two or more dimensions is Q6_K (ggml type 14), token_embd / output
and the lfm2 in_proj / out_proj included; norms and conv taps stay F32; a row length that is no
multiple of 256 falls back to Q8_0 (the 0.1B width: everything but ffn_down)."""
import numpy as np
import pytest

import miotts_amd as m
import np_ref
import pyoracle
from miotts_amd import gguf_np

# SynthLlmCfg::qtype of every preset (csrc/testlib/synth_llm.cpp)
PRESET_QTYPE = {0: 8, 1: 15, 2: 8, 3: 15, 4: 8, 5: 8, 6: 8, 7: 8, 8: 15, 9: 15, 10: 2, 11: 30, 12: 30, 13: 17, 14: 16,
                15: 17, 16: 17, 17: 15, 18: 8}


def _types(path):
    g = gguf_np.GGUFReader(path)
    return g, {t.name: t.type for t in g.tensors}


def test_preset_1_as_q6k(tmp_path):
    g, ty = _types(m.synth_llm_as(str(tmp_path / "a.gguf"), 1, 18, 1))
    assert g.kv["general.file_type"] == 18
    assert set(ty.values()) == {0, 14}
    for name, t in ty.items():
        dims = next(x for x in g.tensors if x.name == name).ne
        assert t == (14 if len(dims) >= 2 else 0), (name, t)
    assert ty["token_embd.weight"] == 14 and "output.weight" not in ty


def test_576_width_falls_back_to_q8_0(tmp_path):
    """Preset 9 (n_embd 576, n_ff 1536): what the published 0.1B Q6_K file holds."""
    g, ty = _types(m.synth_llm_as(str(tmp_path / "a.gguf"), 9, 18, 1))
    assert g.kv["general.file_type"] == 18
    assert ty["token_embd.weight"] == 8
    for il in range(3):
        for n in ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up"):
            assert ty[f"blk.{il}.{n}.weight"] == 8, (il, n)
        assert ty[f"blk.{il}.ffn_down.weight"] == 14
    assert set(ty.values()) == {0, 8, 14}


def test_lfm2_projections_are_q6k(tmp_path):
    g, ty = _types(m.synth_llm_as(str(tmp_path / "a.gguf"), 8, 18, 1))
    conv = [n for n in ty if "shortconv" in n]
    assert any(n.endswith("in_proj.weight") for n in conv) and any(n.endswith("out_proj.weight") for n in conv)
    for n in conv:
        assert ty[n] == (0 if n.endswith("conv.weight") else 14), (n, ty[n])
    assert set(ty.values()) == {0, 14}


def test_untied_output_is_q6k(tmp_path):
    g, ty = _types(m.synth_llm_as(str(tmp_path / "a.gguf"), 14, 18, 1))
    assert ty["output.weight"] == 14 and ty["token_embd.weight"] == 14
    assert set(ty.values()) == {0, 14}


@pytest.mark.parametrize("qtype", [19, 3, 0, -1, 14])
def test_unknown_recipe_is_refused(tmp_path, qtype):
    with pytest.raises(m.HipError, match="unknown recipe"):
        m.synth_llm_as(str(tmp_path / "x.gguf"), 1, qtype, 1)
    with pytest.raises(m.HipError, match="bad args"):
        m.synth_llm_as(str(tmp_path / "x.gguf"), 19, 18, 1)


def test_check_refusals_are_reported(tmp_path):
    """synth_llm_check's refusal (Q5_K at a width that is no multiple of 256) as synth_llm reports it."""
    with pytest.raises(m.HipError, match="multiples of 256"):
        m.synth_llm_as(str(tmp_path / "x.gguf"), 9, 17, 1)


@pytest.mark.parametrize("preset", [0, 1, 5, 8, 9, 10, 11, 13, 14, 17])
def test_own_qtype_writes_the_presets_bytes(tmp_path, preset):
    a = m.synth_llm(str(tmp_path / "a.gguf"), preset, 3)
    b = m.synth_llm_as(str(tmp_path / "b.gguf"), preset, PRESET_QTYPE[preset], 3)
    assert open(a, "rb").read() == open(b, "rb").read()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


def test_oracle_matches_numpy_restatement(tmp_path):
    """tests/test_np_crosscheck.py's sweep, positions and bounds (its tiny Q4_K_M model: 40
    positions, at most 2 layer outputs off by > 2e-5, none by 3e-2) on preset 1 as Q6_K: the two
    CPU references alone stay far inside the 12 % cap the GPU tests put on such flips."""
    path = m.synth_llm_as(str(tmp_path / "a.gguf"), 1, 18, 1)
    n_pos = 40
    o = pyoracle.Llm(path, n_pos)
    n = np_ref.DecodeStep(path, n_pos)
    rng = np.random.default_rng(1)
    toks = [256, 257] + [int(t) for t in rng.integers(260, 13060, n_pos - 2)]
    worst, flips, evals = 0.0, 0, 0
    for pos, t in enumerate(toks):
        x = o.embed(t)
        assert np.array_equal(x, n.embed(t).astype(np.float32))  # a Q6_K embedding row
        for il in range(o.n_layer):
            k, v = o.kv(il, pos)
            n.kc[il, :, :pos], n.vc[il, :, :pos] = k, v
            y_o = o.layer(il, pos, x)
            e = _rel(n.layer(il, x, pos), y_o)
            worst = max(worst, e)
            flips += e > 2e-5
            evals += 1
            x = y_o
        if pos % 8 == 7:
            lo, ln = o.head(x), n.out @ np_ref.rms_norm(x, n.out_norm, n.eps)
            assert _rel(ln, lo) < 2e-5, (pos, _rel(ln, lo))
    print(f"{evals} layer evaluations, {flips} above 2e-5, worst {worst:.3g}")
    assert flips <= 2 and worst < 3e-2, (flips, worst)
