"""CPU: Q3_K (ggml type 11) on the host: the dequantizer against the numpy restatement (np_q3k), the
quantizer against a baseline written out here, the Q3_K_S / Q3_K_M / Q3_K_L recipes of the synthetic
writer, the split layout's round trip, and np_ref.DecodeStep with np_q3k.Mat on the files the GPU
tests use."""
import numpy as np
import pytest

import miotts_amd as m
import np_q3k
import np_ref
from miotts_amd import gguf_np


def _rows(k, n=24, seed=5):
    return (0.05 * np.random.default_rng(seed + k).standard_normal((n, k))).astype(np.float32)


@pytest.mark.parametrize("k", [256, 768, 2048])
def test_dequantize_rows_equals_numpy_bit_for_bit(k):
    raw = m.quantize_rows(11, _rows(k))
    assert raw.shape == (24, k // 256 * 110)
    got = m.dequantize_rows(11, raw, k)
    want = np_q3k.dequant(11, raw, 24, k)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_known_answer_block():
    blk, want = np_q3k.known_answer_block()
    d, s, q = np_q3k.codes(blk, 1, 256)
    assert d[0, 0] == 1.0 and np.array_equal(s[0, 0], (5 * np.arange(16) + 3) % 64)
    assert np.array_equal(np_q3k.dequant(11, blk, 1, 256)[0], want)
    assert np.array_equal(m.dequantize_rows(11, blk.reshape(1, -1), 256)[0], want)
    # the ceiling block: every weight is (-32) * (-4)
    assert np.array_equal(m.dequantize_rows(11, np_q3k.ceiling_block().reshape(1, -1), 256)[0], np.full(256, 128.0))


def _baseline(x):
    """The baseline quantizer, dequantized: per 16-group scale = max|w| / 4, d = max scale / 31 as
    f16, 6-bit scale = round(scale / d), q = clip(round(w / (d * s)), -4, 3)."""
    out = np.zeros_like(x)
    for r in range(x.shape[0]):
        for b in range(x.shape[1] // 256):
            w = x[r, 256 * b:256 * b + 256].reshape(16, 16).astype(np.float64)
            scale = np.abs(w).max(1) / 4
            d = float(np.float16(scale.max() / 31))
            if d == 0:
                continue
            s = np.rint(scale / d)
            dl = d * s
            q = np.clip(np.rint(w / np.where(dl != 0, dl, 1)[:, None]), -4, 3) * (dl != 0)[:, None]
            out[r, 256 * b:256 * b + 256] = (dl[:, None] * q).reshape(-1)
    return out


@pytest.mark.parametrize("k", [256, 768, 2048])
def test_quantizer_is_no_worse_than_the_baseline(k):
    x = _rows(k, n=32, seed=11)
    raw = m.quantize_rows(11, x)
    d, s, q = np_q3k.codes(raw, 32, k)
    assert q.min() >= -4 and q.max() <= 3 and s.min() >= 0 and s.max() <= 63  # valid blocks
    got = m.dequantize_rows(11, raw, k).astype(np.float64)
    rms = lambda y: float(np.sqrt(np.mean((y - x.astype(np.float64)) ** 2)))
    e_cpp, e_base = rms(got), rms(_baseline(x).astype(np.float64))
    print(f"k {k}: rms error {e_cpp:.6g} (baseline {e_base:.6g}, ratio {e_cpp / e_base:.4f})")
    assert e_cpp <= e_base * (1 + 1e-3), (e_cpp, e_base)
    # and close to the N(0, 0.05) rows at all: 3-bit codes, 16-element groups
    assert e_cpp < 0.2 * 0.05


def _types(path):
    g = gguf_np.GGUFReader(path)
    return g, {t.name: t.type for t in g.tensors}


def _want_types(g, ty, recipe, n_layer):
    """llama_tensor_get_type for the three Q3_K file types, by tensor name."""
    attn = sorted({int(n.split(".")[1]) for n in ty if n.endswith("attn_v.weight")})
    for name, t in ty.items():
        dims = next(x for x in g.tensors if x.name == name).ne
        if len(dims) < 2 or name.endswith("shortconv.conv.weight"):
            want = 0
        elif name == "output.weight" or (name == "token_embd.weight" and "output.weight" not in ty):
            want = 14
        elif name.endswith("attn_v.weight"):
            ia = attn.index(int(name.split(".")[1]))
            want = {11: 11, 12: 13 if ia < 2 else 12, 13: 13}[recipe]
        elif name.endswith("attn_output.weight"):
            want = {11: 11, 12: 12, 13: 13}[recipe]
        elif name.endswith("ffn_down.weight"):
            il = int(name.split(".")[1])
            want = {11: 11, 12: 13 if il < n_layer // 16 else 12, 13: 13}[recipe]
        else:  # attn_q, attn_k, ffn_gate, ffn_up, in_proj, out_proj, an untied token_embd
            want = 11
        assert t == want, (recipe, name, t, want)


@pytest.mark.parametrize("recipe", [11, 12, 13])
@pytest.mark.parametrize("preset", [1, 13, 14, 8])
def test_recipe_tensor_types(tmp_path, preset, recipe):
    g, ty = _types(m.synth_llm_as(str(tmp_path / "a.gguf"), preset, recipe, 1))
    assert g.kv["general.file_type"] == recipe
    a = g.kv["general.architecture"]
    _want_types(g, ty, recipe, g.kv[f"{a}.block_count"])
    if preset == 14:  # untied llama: a Q3_K embedding beside a Q6_K output
        assert ty["token_embd.weight"] == 11 and ty["output.weight"] == 14
    if preset == 8:
        assert any(n.endswith("in_proj.weight") and t == 11 for n, t in ty.items())
        assert any(n.endswith("out_proj.weight") and t == 11 for n, t in ty.items())
    if preset == 13 and recipe == 12:  # both attn_v partners of Q3_K_M occur
        assert [ty[f"blk.{i}.attn_v.weight"] for i in range(3)] == [13, 13, 12]


def test_recipe_is_refused_off_256(tmp_path):
    with pytest.raises(m.HipError, match="multiples of 256"):
        m.synth_llm_as(str(tmp_path / "x.gguf"), 9, 12, 1)


def test_split_layout_round_trips():
    """to_split's planes read back by np_q3k.split_inverse (restated from quant.h's table): the
    known-answer block tiled, the ceiling block and quantized random rows."""
    ka, _ = np_q3k.known_answer_block()
    k = 768
    rows = np.stack([np.tile(ka, 3), np.tile(np_q3k.ceiling_block(), 3)] + list(m.quantize_rows(11, _rows(k, n=5))))
    split, off = m.to_split(11, rows, k)
    n = rows.shape[0]
    # 114 bytes per superblock, each plane padded to 256 bytes
    assert off[0] == 0 and off[1] >= n * k // 4 and off[2] >= off[1] + n * k // 8 and off[3] >= off[2] + n * k // 16
    assert n * (k // 256) * 114 <= split.size <= n * (k // 256) * 114 + 4 * 256
    d, sc, q = np_q3k.split_inverse(split, off, n, k)
    d0, s0, q0 = np_q3k.codes(rows, n, k)
    assert np.array_equal(d, d0) and np.array_equal(sc, s0 - 32) and np.array_equal(q, q0)
    e = np.arange(256)
    assert np.array_equal(q[0, 1], (7 * e + 3 * (e // 16)) % 8 - 4)


@pytest.mark.parametrize("preset,recipe", [(13, 12), (14, 11), (8, 12), (17, 13)])
def test_numpy_decode_step_reads_the_files(tmp_path, monkeypatch, preset, recipe):
    """np_ref.DecodeStep with np_q3k.Mat loads each file of the GPU layer test and runs layers."""
    monkeypatch.setattr(np_ref, "Mat", np_q3k.Mat)
    path = m.synth_llm_as(str(tmp_path / "a.gguf"), preset, recipe, 1)
    n = np_ref.DecodeStep(path, 8)
    x = n.embed(300)
    raw = gguf_np.GGUFReader(path).tensor("token_embd.weight")
    if raw.type == 11:
        assert np.array_equal(x, np_q3k.dequant(11, raw.raw(), raw.ne[1], raw.ne[0])[300])
    for il in range(n.n_layer):
        x = n.layer(il, x, 0)
    assert x.shape == (n.n_embd,) and np.all(np.isfinite(x)) and float(np.abs(x).max()) > 0
