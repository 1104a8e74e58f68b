"""Decode-step cost of the 1.7B shape as Q4_K_M (preset 3), Q5_K_M (preset 16), Q6_K (preset 3
written as MOSTLY_Q6_K), Q3_K_M and Q3_K_S (preset 3 written with recipes 12 and 11), one process;
--shape 2.6B / 0.1B: that shape as Q8_0 and as Q6_K.

All models are loaded, then timed alternately (REPS rounds): HIP events around a free-running
generate() of N_LONG tokens and one of N_SHORT tokens from the same prompt and seed; the
difference is (steps issued long - short) >= 200 graph-replayed decode steps with the prompt
prefill and the start-up cancelled. The same positions are decoded for every model. Reported per
model: ms per step (best round and all rounds), mio_hip_llm_weight_bytes (the bytes a step
streams) and the HBM fraction = weight bytes / step time / 8 TB/s, plus each launch kind's
event time and bytes (mio_hip_llm_time_kernel) to tell which launch a difference comes from.
The batched leg times generate_batch of BATCH streams the same way (events, long minus short, no
end token: every stream decodes every step) and reports ms per batched step and the launches
one such step issues. The fusion switches of the environment (MIO_LAYER_ATT, MIO_ATT_FUSE_O,
MIO_FFN_FUSE) are recorded: a run with the three at 0 is the separate-launch arm.

  python tools/bench_quant_types.py [--shape 1.7B] [--out profiles/q6k_step.json]

Needs a GPU; writes the JSON and prints it. bench.py is not involved."""
import argparse
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "miotts-llama.cpp_amd", "python"))
import numpy as np  # noqa: E402

import miotts_amd as m  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E
N_SHORT, N_LONG, REPS = 64, 464, 3
BATCH, B_SHORT, B_LONG = 8, 32, 232
# shape -> (name, preset, recipe or None for the preset's own)
SHAPES = {"1.7B": (("q4_K_M", 3, None), ("q5_K_M", 16, None), ("q6_K", 3, 18), ("q3_K_M", 3, 12), ("q3_K_S", 3, 11)),
          "2.6B": (("q8_0", 4, None), ("q6_K", 4, 18)),
          "0.1B": (("q8_0", 2, None), ("q6_K", 2, 18))}
SWITCHES = ("MIO_LAYER_ATT", "MIO_ATT_FUSE_O", "MIO_FFN_FUSE")
KINDS = m.STEP_KIND_NAMES


def timed_generate(dev, llm, prompt, n, allow):
    dev.mark(0)
    toks = llm.generate(prompt, n, 0.8, 7, allow=allow, check_interval=32)
    dev.mark(1)
    assert len(toks) == n, (len(toks), n)
    return dev.elapsed_ms(0, 1), llm.steps_issued()


def timed_batch(dev, llm, prompts, n, allow):
    dev.mark(0)
    toks = llm.generate_batch(prompts, n, 0.8, [7 + b for b in range(len(prompts))], allow=allow)
    dev.mark(1)
    assert all(len(t) == n for t in toks), [len(t) for t in toks]
    return dev.elapsed_ms(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "q6k_step.json"))
    ap.add_argument("--shape", default="1.7B", choices=sorted(SHAPES))
    ap.add_argument("--dir", default=None, help="where the synthetic GGUFs go (default: a temporary directory)")
    a = ap.parse_args()
    if m.device_count() < 1:
        sys.exit("bench_quant_types: no GPU")
    dev = m.Device(0)
    allow = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800)
    prompt = np.array([256, 257, 65, 258, 257, 300, 301], np.int32)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        models = {}
        prompts = [list(prompt) for _ in range(BATCH)]
        for name, preset, recipe in SHAPES[a.shape]:
            path = os.path.join(d, f"llm{preset}_{name}.gguf")
            path = m.synth_llm(path, preset, 1) if recipe is None else m.synth_llm_as(path, preset, recipe, 1)
            llm = m.Llm(dev, path, 2048)
            timed_generate(dev, llm, prompt, N_LONG, allow)  # warm-up: code objects, graphs, every position
            timed_batch(dev, llm, prompts, B_LONG, allow)
            models[name] = {"preset": preset, "recipe": recipe, "llm": llm, "ms": [], "bms": []}
        for _ in range(REPS):
            for r in models.values():
                t0, s0 = timed_generate(dev, r["llm"], prompt, N_SHORT, allow)
                t1, s1 = timed_generate(dev, r["llm"], prompt, N_LONG, allow)
                assert s1 - s0 >= 200, (s0, s1)
                r["steps"] = s1 - s0
                r["ms"].append((t1 - t0) / (s1 - s0))
        for _ in range(REPS):
            for r in models.values():
                b0 = timed_batch(dev, r["llm"], prompts, B_SHORT, allow)
                b1 = timed_batch(dev, r["llm"], prompts, B_LONG, allow)
                r["bms"].append((b1 - b0) / (B_LONG - B_SHORT))
        out = {"workload": f"{a.shape} shape, free-running decode, steps {N_SHORT}..{N_LONG} after a {len(prompt)}-token "
                           f"prompt, graph-replayed, HIP events, {REPS} alternating rounds; batched: {BATCH} streams, "
                           f"steps {B_SHORT}..{B_LONG}",
               "box": os.uname().nodename,
               "switches": {k: os.environ.get(k, "") for k in SWITCHES},
               "hbm_peak_GBps": HBM_PEAK_GBS, "models": {}}
        for name, r in models.items():
            llm = r["llm"]
            ms, wb = min(r["ms"]), llm.weight_bytes()
            kinds = llm.step_kinds()
            per = {}
            for which in sorted(set(kinds)):
                kms, by = llm.time_kernel(which, 100)
                per[KINDS.get(which, str(which))] = {"launches_per_step": kinds.count(which), "event_us": round(kms * 1e3, 3),
                                                     "bytes": int(by)}
            bms = min(r["bms"])
            out["models"][name] = {"preset": r["preset"], "recipe": r["recipe"], "steps_timed": r["steps"],
                                   "ms_per_step": round(ms, 5),
                                   "ms_per_step_rounds": [round(v, 5) for v in r["ms"]], "weight_bytes": int(wb),
                                   "hbm_frac": round(wb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                   "launches_per_step": len(kinds), "launches": per,
                                   "batch": {"streams": BATCH, "ms_per_step": round(bms, 5),
                                             "ms_per_step_rounds": [round(v, 5) for v in r["bms"]],
                                             "hbm_frac": round(wb / (bms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                             "launches_per_step": llm.batch_step_launches(BATCH)}}
            llm.close()
        names = [n for n, _, _ in SHAPES[a.shape]]
        base = out["models"][names[0]]
        for n in names[1:]:
            o = out["models"][n]
            out[f"{n}_over_{names[0]}"] = {"ms_per_step": round(o["ms_per_step"] / base["ms_per_step"], 4),
                                           "weight_bytes": round(o["weight_bytes"] / base["weight_bytes"], 4),
                                           "hbm_frac": round(o["hbm_frac"] / base["hbm_frac"], 4),
                                           "batch_ms_per_step": round(o["batch"]["ms_per_step"] /
                                                                      base["batch"]["ms_per_step"], 4)}
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
