"""GPU: the decode step's fused attention launches let the chunk that owns `pos` merge its kv head's
records (attn_merge_owner, csrc/hip/llm_device.h), and k_layer_att's chunks wait for the head rows
they load only (a q row counter beside the q|k|v row counter per kv head). Neither changes a bit:

1. on a cache filled with set_kv_rows in every layer, the logits of `eval` are bit-identical between
   k_layer_att (MIO_LAYER_ATT=1), attn_in + k_att_o (MIO_LAYER_ATT=0) and the separate launches
   (MIO_ATT_FUSE_O=0 MIO_FFN_FUSE=0, the ticket merge) at the positions where the merge changes
   shape: 0 (one chunk, no wait), 1, 63, 64 (the owner holds one position), 65, 127, 128, 511, 512,
   513 (the merge's 8-chunk batch edge), 575, 576 and n_ctx - 1 of a 1024-position context, for
   the three head shapes with a fused launch: (hd 64, 3 query heads per kv head) preset 9,
   (128, 2) and (64, 4). The tiny presets of the last two, 17 and 18, have no k_layer_att at their
   widths (their steps hold kind 10 and never 11, whatever MIO_LAYER_ATT says), so k_layer_att
   runs on the smallest presets of those head shapes that have it, 3 (1.7B) and 4 (2.6B), and
   17 and 18 compare k_att_o with the separate launches;
2. 2,000 free-run decode steps of preset 9 on k_layer_att end without a hand-off timeout
   (generate raises HipError on one) with the separate launches' tokens;
3. after those runs, and after the runner's counter reset, the q row counters, the q|k|v row
   counters and the arrival words read 0.

Every variant is a fresh process (the switches are read once) under its own time limit; a
variant's run is made once and shared by the tests that need it.
"""
import functools
import json
import os
import subprocess
import sys

import pytest

import miotts_amd as m

pytestmark = pytest.mark.gpu

N_CTX = 1024
POSITIONS = (0, 1, 63, 64, 65, 127, 128, 511, 512, 513, 575, 576, N_CTX - 1)
SOAK_STEPS = 2000
VARIANTS = {
    "layer_att": {"MIO_LAYER_ATT": "1"},
    "att_o": {"MIO_LAYER_ATT": "0"},
    "separate": {"MIO_ATT_FUSE_O": "0", "MIO_FFN_FUSE": "0"},
}

_SCRIPT = """
import hashlib
import json
import sys
sys.path.insert(0, sys.argv[2])
import numpy as np
import miotts_amd as m
mode, n_ctx = sys.argv[3], int(sys.argv[4])
dev = m.Device(0)
g = m.Llm(dev, sys.argv[1], n_ctx)
out = {"kinds": g.step_kinds()}
if mode == "logits":
    rng = np.random.default_rng(7)
    k = (0.5 * rng.standard_normal((g.n_kv, n_ctx, g.head_dim))).astype(np.float16)
    v = (0.5 * rng.standard_normal((g.n_kv, n_ctx, g.head_dim))).astype(np.float16)
    for il in range(g.n_layer):  # every layer its own rows: the same ones, il positions on
        g.set_kv_rows(il, 0, np.roll(k, il, axis=1), np.roll(v, il, axis=1))
    out["digests"] = {}
    for pos in json.loads(sys.argv[5]):
        lg = g.eval(5 + pos % 7, pos)
        assert np.isfinite(lg).all(), pos
        out["digests"][str(pos)] = hashlib.sha256(lg.tobytes()).hexdigest()
else:
    tok = g.generate([256, 257, 84, 101, 115, 116, 258, 257], int(sys.argv[5]), 0.8, 42,
                     allow=(m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800))
    out["n_tokens"] = int(len(tok))
    out["tokens"] = hashlib.sha256(np.asarray(tok, np.int32).tobytes()).hexdigest()
out["words"] = g.handoff_words().reshape(-1).tolist()
out["words_reset"] = g.handoff_words(reset=True).reshape(-1).tolist()
print(json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def _script(tmp):
    path = os.path.join(tmp, "owner_merge_child.py")
    with open(path, "w") as f:
        f.write(_SCRIPT)
    return path


@functools.lru_cache(maxsize=None)
def _run(tmp, path, variant, mode):
    pkg = os.path.dirname(os.path.dirname(m.__file__))
    n_ctx = N_CTX if mode == "logits" else SOAK_STEPS + 48
    arg = json.dumps(list(POSITIONS)) if mode == "logits" else str(SOAK_STEPS)
    p = subprocess.run([sys.executable, _script(tmp), path, pkg, mode, str(n_ctx), arg], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, **VARIANTS[variant]))
    assert p.returncode == 0, (variant, mode, p.stdout[-1000:] + p.stderr[-3000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("owner_merge"))


# (preset, its step holds k_layer_att under MIO_LAYER_ATT=1)
CASES = [(9, True), (17, False), (18, False), (3, True), (4, True)]


def _variants(has11):
    return [v for v in VARIANTS if has11 or v != "layer_att"]


def _check_kinds(outs):
    if "layer_att" in outs:
        assert 11 in outs["layer_att"]["kinds"], outs["layer_att"]["kinds"]
    assert 10 in outs["att_o"]["kinds"] and 11 not in outs["att_o"]["kinds"], outs["att_o"]["kinds"]
    assert not {10, 11, 12} & set(outs["separate"]["kinds"]), outs["separate"]["kinds"]


@pytest.mark.parametrize("preset,has11", CASES)
def test_logits_bit_identical_across_launch_forms(synth_llm_path, tmp, preset, has11):
    path = synth_llm_path(preset)
    outs = {v: _run(tmp, path, v, "logits") for v in _variants(has11)}
    _check_kinds(outs)
    ref = outs["separate"]["digests"]
    assert sorted(map(int, ref)) == sorted(POSITIONS)
    for v in _variants(has11)[:-1]:
        differ = [pos for pos in POSITIONS if outs[v]["digests"][str(pos)] != ref[str(pos)]]
        print(preset, v, "positions that differ from the separate launches:", differ)
        assert not differ, (preset, v, differ)


def test_handoff_soak(synth_llm_path, tmp):
    path = synth_llm_path(9)
    outs = {v: _run(tmp, path, v, "soak") for v in ("layer_att", "separate")}
    assert 11 in outs["layer_att"]["kinds"] and not {10, 11, 12} & set(outs["separate"]["kinds"])
    print({v: (o["n_tokens"], o["tokens"]) for v, o in outs.items()})
    assert outs["layer_att"]["n_tokens"] == outs["separate"]["n_tokens"] == SOAK_STEPS
    assert outs["layer_att"]["tokens"] == outs["separate"]["tokens"]


def test_counter_words_read_zero(synth_llm_path, tmp):
    runs = [(preset, v, "logits") for preset, has11 in CASES for v in _variants(has11)[:-1]] + [(9, "layer_att", "soak")]
    for preset, v, mode in runs:
        o = _run(tmp, synth_llm_path(preset), v, mode)
        assert o["words"] and not any(o["words"]), (preset, v, mode, o["words"])
        assert o["words_reset"] and not any(o["words_reset"]), (preset, v, mode, o["words_reset"])
