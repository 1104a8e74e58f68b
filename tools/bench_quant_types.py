"""Decode-step cost of the 1.7B shape as Q4_K_M (preset 3) and as Q5_K_M (preset 16), one process.

Both models are loaded, then timed alternately (REPS rounds): HIP events around a free-running
generate() of N_LONG tokens and one of N_SHORT tokens from the same prompt and seed; the
difference is (steps issued long - short) >= 200 graph-replayed decode steps with the prompt
prefill and the start-up cancelled. The same positions are decoded for both models. Reported per
model: ms per step (best round and all rounds), mio_hip_llm_weight_bytes (the bytes a step
streams) and the HBM fraction = weight bytes / step time / 8 TB/s, plus each launch kind's
event time and bytes (mio_hip_llm_time_kernel) to tell which launch a difference comes from.

  python tools/bench_quant_types.py [--out profiles/q5k_step.json]

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
KINDS = m.STEP_KIND_NAMES


def timed_generate(dev, llm, prompt, n, allow):
    dev.mark(0)
    toks = llm.generate(prompt, n, 0.8, 7, allow=allow, check_interval=32)
    dev.mark(1)
    assert len(toks) == n, (len(toks), n)
    return dev.elapsed_ms(0, 1), llm.steps_issued()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "q5k_step.json"))
    ap.add_argument("--dir", default=None, help="where the synthetic GGUFs go (default: a temporary directory)")
    a = ap.parse_args()
    if m.device_count() < 1:
        sys.exit("bench_quant_types: no GPU")
    dev = m.Device(0)
    allow = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800)
    prompt = np.array([256, 257, 65, 258, 257, 300, 301], np.int32)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        models = {}
        for name, preset in (("q4_K_M", 3), ("q5_K_M", 16)):
            llm = m.Llm(dev, m.synth_llm(os.path.join(d, f"llm{preset}.gguf"), preset, 1), 2048)
            timed_generate(dev, llm, prompt, N_LONG, allow)  # warm-up: code objects, graphs, every position
            models[name] = {"preset": preset, "llm": llm, "ms": []}
        for _ in range(REPS):
            for r in models.values():
                t0, s0 = timed_generate(dev, r["llm"], prompt, N_SHORT, allow)
                t1, s1 = timed_generate(dev, r["llm"], prompt, N_LONG, allow)
                assert s1 - s0 >= 200, (s0, s1)
                r["steps"] = s1 - s0
                r["ms"].append((t1 - t0) / (s1 - s0))
        out = {"workload": f"1.7B shape, free-running decode, steps {N_SHORT}..{N_LONG} after a {len(prompt)}-token "
                           f"prompt, graph-replayed, HIP events, {REPS} alternating rounds",
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
            out["models"][name] = {"preset": r["preset"], "steps_timed": r["steps"], "ms_per_step": round(ms, 5),
                                   "ms_per_step_rounds": [round(v, 5) for v in r["ms"]], "weight_bytes": int(wb),
                                   "hbm_frac": round(wb / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "launches": per}
            llm.close()
        a4, a5 = out["models"]["q4_K_M"], out["models"]["q5_K_M"]
        out["q5_over_q4"] = {"ms_per_step": round(a5["ms_per_step"] / a4["ms_per_step"], 4),
                             "weight_bytes": round(a5["weight_bytes"] / a4["weight_bytes"], 4),
                             "hbm_frac": round(a5["hbm_frac"] / a4["hbm_frac"], 4)}
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
