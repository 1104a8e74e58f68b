"""GPU: the decode kernels give, behind their entry pack (csrc/hip/llm_device.h, "kernel entry"),
the bytes they gave before it.

tests/golden/entry_args_parent.npz was recorded on the MI355X by tools/record_entry_args.py at
db4e6ca, the commit before the pack; that file describes the models and the cases (its runner is
used here, so both sides run the same inputs). Every model runs twice, each in a fresh process
(the switch is read once): with graph replay, where every kernel node stores its own copy of the
arguments, and with eager launches (MIO_NO_GRAPH=1). Every comparison is bytewise."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_entry_args as R  # noqa: E402

pytestmark = pytest.mark.gpu

# launch kinds (miotts_amd.STEP_KIND_NAMES) each model's step must hold, so that every signature
# with a pack is reached: 0 k_attn_in, 10 k_att_o, 11 k_layer_att, 12 k_ffn, 6 k_lm_head, 8 k_attn_in
# over an lfm2 in_proj
KINDS = {17: {0, 10, 11, 12, 6}, 9: {0, 10, 6}, 8: {8, 0, 6}}


@pytest.fixture(scope="module")
def golden():
    with np.load(R.FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """runs(preset, mode) -> the arrays of tools/record_entry_args.py --preset, run once per
    (preset, mode) in a child process; mode "graph" or "eager"."""
    d = tmp_path_factory.mktemp("entry_args")
    cache = {}

    def get(preset, mode):
        if (preset, mode) not in cache:
            out = str(d / f"p{preset}_{mode}.npz")
            env = dict(os.environ, MIO_NO_GRAPH="1" if mode == "eager" else "0")
            p = subprocess.run([sys.executable, os.path.join(R.REPO, "tools", "record_entry_args.py"), "--preset",
                                str(preset), "--out", out], capture_output=True, text=True, timeout=120, env=env)
            assert p.returncode == 0, p.stderr[-2000:]
            with np.load(out) as z:
                cache[preset, mode] = {k: z[k] for k in z.files}
        return cache[preset, mode]

    return get


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (
        what, got.shape, want.shape, int((got != want).sum()) if got.shape == want.shape else -1)


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("preset", R.PRESETS)
def test_tokens_and_logits(runs, golden, preset, mode):
    """(a), (b): 24 tokens and the last step's logits, graph replay and eager launches."""
    r = runs(preset, mode)
    assert KINDS[preset] <= set(r["kinds"].tolist()), r["kinds"]
    _same(r["kinds"], golden[f"p{preset}_kinds"], "kinds")
    _same(r["tok24"], golden[f"p{preset}_tok24"], "tokens")
    _same(r["logits24"], golden[f"p{preset}_logits24"], "logits")


@pytest.mark.parametrize("mode", ["graph", "eager"])
@pytest.mark.parametrize("preset", R.PRESETS)
def test_end_token_inside_the_run(runs, golden, preset, mode):
    """(c): the run stops at the fixture's end token; the steps queued past it (tail() counts them)
    returned at entry, i.e. the logits buffer is still what the end token's step wrote (the `done`
    flag is read through the pack); layer 0's k_ffn still folded the end token's step, so the run
    that follows on the same handle gives the first run's bytes again."""
    r = runs(preset, mode)
    _same(r["eos_tok"], golden[f"p{preset}_eos_tok"], "tokens before the end token")
    assert len(r["eos_tok"]) < 200
    wasted, tail0 = (int(v) for v in r["eos_wasted"])
    # eager launches stop at the next host check, graph replay runs up to two 8-step graphs ahead
    assert wasted == tail0 and wasted >= 1, (wasted, tail0)
    _same(r["eos_logits"], golden[f"p{preset}_eos_logits"], "logits after the end token")
    _same(r["again_tok"], golden[f"p{preset}_tok24"], "tokens of the following run")
    _same(r["again_logits"], golden[f"p{preset}_logits24"], "logits of the following run")


@pytest.mark.parametrize("preset", R.PRESETS)
def test_diagnostic_instantiations(runs, golden, preset):
    """(d): the last three of the 24 steps on the DG instantiations (a timeline buffer attached):
    the 24th step's logits, which depend on every token sampled before, are the plain run's."""
    r = runs(preset, "graph")
    _same(r["dg_logits"], golden[f"p{preset}_dg_logits"], "logits behind the timeline steps")
    _same(r["dg_logits"], golden[f"p{preset}_logits24"], "logits behind the timeline steps")
