"""Records what the decode step gives on the tiny presets that reach every decode-kernel
signature, as bit patterns:
    python tools/record_entry_args.py            (on the GPU, at the commit to pin)
writes tests/golden/entry_args_parent.npz, which tests/test_entry_args_gpu.py compares with byte
for byte. The fixture in the tree was written at db4e6ca, the commit before the decode kernels
took their entry pack (the leading scalar and pointer parameters their first loads are issued
from): that change may not move a bit.

    python tools/record_entry_args.py --preset P --out FILE
runs one preset's cases in this process and writes them to FILE (the test starts it once with
graph replay and once with MIO_NO_GRAPH=1: the switch is read once per process).

Models (no tiny preset has a shape the fused launches are instantiated for, so the first is preset
17 at sizes of its own, the smallest that pick the 1.7B model's instantiations):
  17  hd 128, G 2, Q4_K_M, n_embd 256, 3 layers, 16 heads over 8 kv heads, n_ff 6144: k_attn_in +
      k_att_o in layer 0, k_layer_att in the others, k_ffn in all (attn_v / ffn_down Q4_K and
      Q6_K both occur), k_lm_head
  9   hd 64, G 3, Q4_K_M: k_attn_in + k_att_o in every layer, the separate FFN launches
  8   lfm2 Q4_K_M: k_attn_in over in_proj + k_conv_out, the separate attention launches
Per model:
  tok24, logits24    24 free-run tokens and the last step's logits
  eos_tok, eos_logits  a run that samples an end token (1 in 4 allowed ids, temperature 2): the
                     tokens before it, and the logits buffer afterwards, which the steps queued
                     past the end token must leave as the end token's step wrote it
  again_tok, again_logits  the first run again on the same handle
  dg_logits          (graph replay only) 21 tokens, then three steps on the diagnostic
                     instantiations (mio_hip_llm_timeline), then the logits buffer: the 24th
                     step's, so the same bytes as logits24
  kinds              the step's launch kinds"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_p = os.path.join(REPO, "miotts-llama.cpp_amd", "python")
if _p not in sys.path:
    sys.path.insert(0, _p)
import miotts_amd as m  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "entry_args_parent.npz")
PRESETS = (17, 9, 8)
N_CTX = 256
N_TOK = 24
N_DG = 3  # steps mio_hip_llm_timeline replays
PROMPT = (256, 257, 65, 258, 257, 300, 301)
EOS_SEED = 11


SHAPES = {17: dict(qtype=15, n_embd=256, n_layer=3, n_head=16, n_head_kv=8, n_ff=6144)}


def model_file(d, preset):
    path = os.path.join(d, f"llm{preset}.gguf")
    if preset in SHAPES:
        return m.synth_llm_shape(path, preset, seed=1, **SHAPES[preset])
    return m.synth_llm(path, preset, 1)


def free_run(g, n):
    toks = g.generate(list(PROMPT), n, 0.8, 5, allow=(m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800), check_interval=16)
    return np.asarray(toks, np.int32), g.logits().view(np.uint32)


def eos_run(g):
    """(tokens before the end token, logits buffer afterwards, steps issued past the end token,
    the same from tail())."""
    toks = g.generate(list(PROMPT), 200, 2.0, EOS_SEED, allow=(m.SYNTH_EOT, m.SYNTH_SPEECH0 + 3),
                      eos=(m.SYNTH_EOT, m.SYNTH_IM_END), check_interval=16)
    wasted = g.steps_issued() - len(toks) - 1
    return np.asarray(toks, np.int32), g.logits().view(np.uint32), wasted, g.tail()[0]


def run_cases(path, dg):
    dev = m.Device(0)
    g = m.Llm(dev, path, N_CTX)
    out = {"kinds": np.asarray(g.step_kinds(), np.int32)}
    out["tok24"], out["logits24"] = free_run(g, N_TOK)
    out["eos_tok"], out["eos_logits"], wasted, tail0 = eos_run(g)
    out["eos_wasted"] = np.asarray([wasted, tail0], np.int32)
    out["again_tok"], out["again_logits"] = free_run(g, N_TOK)
    if dg:
        free_run(g, N_TOK - N_DG)
        t = g.timeline()
        assert t.shape[0] == len(out["kinds"]), t.shape
        out["dg_logits"] = g.logits().view(np.uint32)
    g.close()
    dev.close()
    return out


def main():
    import tempfile

    p = argparse.ArgumentParser()
    p.add_argument("--preset", type=int, default=None)
    p.add_argument("--model", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    dg = os.environ.get("MIO_NO_GRAPH", "0") != "1"
    with tempfile.TemporaryDirectory() as d:
        if a.preset is not None:
            path = a.model or model_file(d, a.preset)
            np.savez_compressed(a.out, **run_cases(path, dg))
            return
        rec = {}
        for preset in PRESETS:
            path = model_file(d, preset)
            r = run_cases(path, dg)
            print(f"preset {preset}: kinds {r['kinds'].tolist()}, {len(r['eos_tok'])} tokens before the end token, "
                  f"{r['eos_wasted'].tolist()} steps after it, again == first {np.array_equal(r['again_logits'], r['logits24'])}, "
                  f"dg == first {np.array_equal(r['dg_logits'], r['logits24'])}")
            for k, v in r.items():
                if k != "eos_wasted":  # how far the host ran ahead: timing, not a result
                    rec[f"p{preset}_{k}"] = v
    dst = a.out or FIXTURE
    np.savez_compressed(dst, **rec)
    print(f"{dst}: {len(rec)} arrays, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
