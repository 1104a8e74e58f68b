"""GPU: the LLM runner's diagnostics (csrc/host/llm_diag.cpp) and the loader's refusals.

time_kernel and trace_kernel take a step kind (miotts_amd.STEP_KIND_NAMES) and run it on the
layer the runner picks for it. Checked on tiny models at n_ctx 128:
1. both accept every kind the model's step has, both refuse (HipError) exactly the kinds no layer
   of the model can run, and they differ only in kind 7 (the flush sampler: traced, not timed).
   Presets 17, 9 and 7 have kinds {0, 1, 2, 3, 4, 6, 8, 9, 10, 12} between them: no tiny preset
   runs kind 11 (k_layer_att) under the default policy, which keeps preset 9's head shape on
   attn_in + k_att_o, and the preset list is closed (test_presets_end_at_18). Kind 11 is reached
   on preset 9 with MIO_LAYER_ATT=1 ("wherever instantiated"), in a fresh process like the
   unfused step (MIO_ATT_FUSE_O=0 MIO_FFN_FUSE=0, kinds 1..4 on preset 17);
2. neither changes what the next generate / eval computes (the decode state is put back);
3. the byte model time_kernel returns equals the recorded one (tests/golden/step_kind_bytes.json);
4. a load refused after the model object exists (n_ctx above the maximum) leaves the device
   usable: the next load of the same file works.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import miotts_amd as m

pytestmark = pytest.mark.gpu

# 17: hd 128, 2 query heads per kv head, Q4_K_M; 9: hd 64, 3 query heads per kv head; 7: tiny lfm2
PRESETS = (17, 9, 7)
N_CTX = 128
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_kind_bytes.json")


def _accepts(call):
    try:
        call()
        return True
    except m.HipError:
        return False


def diag_sets(g):
    """(kinds of the step, kinds time_kernel accepts, kinds trace_kernel accepts), after checking
    them against each other and against what the step says the model can run."""
    kinds = set(g.step_kinds())
    timeable = {k for k in range(14) if _accepts(lambda: g.time_kernel(k, 2))}
    traceable = {k for k in range(14) if _accepts(lambda: g.trace_kernel(k))}
    assert kinds <= timeable and kinds <= traceable, (kinds, timeable, traceable)
    # what a layer of this model can run: the unfused launches of its layer sorts, and each fused
    # launch the step uses or that a more fused launch of the step is made of
    can = {0, 1, 2, 3, 4, 6} | ({8, 9} if 8 in kinds else set())
    can |= ({10} if kinds & {10, 11, 13} else set()) | ({11} if kinds & {11, 13} else set())
    can |= ({12} if kinds & {12, 13} else set()) | ({13} if 13 in kinds else set())
    assert timeable == can, (sorted(kinds), sorted(timeable), sorted(can))
    assert traceable == can | {7}, (sorted(kinds), sorted(traceable), sorted(can))
    return kinds, timeable, traceable


def test_diagnostics_agree_on_what_exists(device, synth_llm_path):
    seen = set()
    for preset in PRESETS:
        g = m.Llm(device, synth_llm_path(preset), N_CTX)
        g.eval(5, 3)
        seen |= diag_sets(g)[0]
        g.close()
    assert seen >= {0, 6, 8, 9, 10, 12}, sorted(seen)  # 11: test_diagnostics_agree_under_switches


_SWITCH_SCRIPT = """
import json
import sys
sys.path[:0] = [sys.argv[2], sys.argv[3]]
import miotts_amd as m
import test_llm_diag_gpu as t
dev = m.Device(0)
g = m.Llm(dev, sys.argv[1], t.N_CTX)
g.eval(5, 3)
t.diag_sets(g)
g.eval(5, 70)
print(json.dumps(t.step_bytes(g)))
"""


def step_bytes(g):
    kinds = g.step_kinds()
    return {"step_kinds": kinds, "bytes": {str(k): int(g.time_kernel(k, 2)[1]) for k in sorted(set(kinds))}}


@pytest.mark.parametrize("preset,env,kinds", [(17, {"MIO_ATT_FUSE_O": "0", "MIO_FFN_FUSE": "0"}, {0, 1, 2, 3, 4, 6}),
                                              (9, {"MIO_LAYER_ATT": "1"}, {0, 3, 4, 6, 10, 11})])
def test_diagnostics_agree_under_switches(synth_llm_path, tmp_path, preset, env, kinds):
    """The same in a fresh process (the switches are read once): the unfused step, where no fused
    kind may be accepted, and k_layer_att (kind 11), whose bytes are compared as well."""
    script = tmp_path / "switches.py"
    script.write_text(_SWITCH_SCRIPT)
    pkg = os.path.dirname(os.path.dirname(m.__file__))
    p = subprocess.run([sys.executable, str(script), synth_llm_path(preset), pkg, os.path.dirname(os.path.abspath(__file__))],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert set(got["step_kinds"]) == kinds, got
    if "MIO_LAYER_ATT" in env:
        assert got == json.load(open(GOLDEN))["presets_MIO_LAYER_ATT_1"][str(preset)]


def test_diagnostics_leave_the_decode_state_alone(device, synth_llm_path):
    g = m.Llm(device, synth_llm_path(17), N_CTX)
    prompt = np.array([256, 257, 65, 258, 257], np.int32)

    def run():
        toks = g.generate(prompt, 24, 0.0, 1)
        return toks, g.eval(int(toks[0]), 40)

    toks0, lg0 = run()
    assert len(toks0) == 24
    for k in sorted(set(g.step_kinds())):
        g.time_kernel(k, 2)
        g.trace_kernel(k)
    toks1, lg1 = run()
    assert np.array_equal(toks0, toks1)
    assert lg0.tobytes() == lg1.tobytes()
    g.close()


def test_byte_model_unchanged(device, synth_llm_path):
    gold = json.load(open(GOLDEN))["presets"]
    for preset in PRESETS:
        g = m.Llm(device, synth_llm_path(preset), N_CTX)
        g.eval(5, 70)
        assert step_bytes(g) == gold[str(preset)], preset
        g.close()


def test_refused_load_then_a_good_one(device, synth_llm_path):
    path = synth_llm_path(1)
    with pytest.raises(m.HipError, match="n_ctx"):
        m.Llm(device, path, 40000)
    g = m.Llm(device, path, N_CTX)
    assert np.isfinite(g.eval(5, 3)).all()
    g.close()
