"""The utterance queue against groups of 16 on a ragged set of utterances, one process, one handle.

64 utterances on the synthetic 1.7B Q4_K_M model (preset 3) at n_ctx 512, ragged by construction:
no end tokens, prompt lengths drawn so that the context-full budgets n_ctx - len + 1 are uniform
in [32, 448] tokens. They are decoded two ways:

  queue   one generate_queue call, 16 slots: a slot whose utterance has ended takes the next one
  groups  four generate_batch calls of 16 utterances in index order: each call lasts as long as
          its longest utterance, the slots of the shorter ones run frozen meanwhile

Both ways prefill the same prompt tokens and sample the same tokens (checked: every utterance is
identical in both). After one warm-up of each (code objects, graphs of the 16-stream step), PAIRS
pairs are timed alternately, queue first in even pairs and groups first in odd ones: a host clock
around calls that end in a device synchronise. Reported: every pair's two times, the median of
the per-pair ratios groups / queue (> 1: the queue is faster), the batched steps each way issued
and the queue's occupancy live_slot_steps / (steps * slots) beside the groups' (the same sum of
sampled steps over 16 x the steps the four calls issued, i.e. the sum of each group's longest
budget: a call's last graph issues only what that budget still takes), and a SHA-256 over every
utterance's tokens as the timed calls return them.

  python tools/queue_bench.py [--out profiles/utt_queue/runs.txt]

Needs a GPU; prints the report and writes it to --out. bench.py is not involved."""
import argparse
import hashlib
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "miotts-llama.cpp_amd", "python"))
import numpy as np  # noqa: E402

import miotts_amd as m  # noqa: E402

N, SLOTS, N_CTX, PAIRS = 64, 16, 512, 5
BUDGET_LO, BUDGET_HI = 32, 448


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "utt_queue", "runs.txt"))
    ap.add_argument("--dir", default=None, help="where the synthetic GGUF goes (default: a temporary directory)")
    a = ap.parse_args()
    if m.device_count() < 1:
        sys.exit("queue_bench: no GPU")
    dev = m.Device(0)
    allow = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800)
    rng = np.random.default_rng(64)
    budgets = [int(b) for b in rng.integers(BUDGET_LO, BUDGET_HI + 1, N)]
    prompts = [list(rng.integers(0, 256, N_CTX + 1 - b)) for b in budgets]
    seeds = [1000 + u for u in range(N)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        llm = m.Llm(dev, m.synth_llm(os.path.join(d, "llm3.gguf"), 3, 1), N_CTX)

        def queue():
            t0 = time.perf_counter()
            toks, stats = llm.generate_queue(prompts, N_CTX, 0.8, seeds, slots=SLOTS, allow=allow)
            return time.perf_counter() - t0, toks, stats

        def groups():
            t0 = time.perf_counter()
            toks = []
            for g0 in range(0, N, SLOTS):
                toks += llm.generate_batch(prompts[g0:g0 + SLOTS], N_CTX, 0.8, seeds[g0:g0 + SLOTS], allow=allow)
            return time.perf_counter() - t0, toks

        _, tq, stats = queue()  # warm-up of both ways, and the outputs compared
        _, tg = groups()
        assert [len(t) for t in tq] == budgets, "the queue's lengths are not the budgets"
        assert all(np.array_equal(x, y) for x, y in zip(tq, tg)), "queue and groups sampled different tokens"
        live = sum(budgets)
        gsteps = sum(max(budgets[g0:g0 + SLOTS]) for g0 in range(0, N, SLOTS))
        say(f"model: synthetic 1.7B Q4_K_M (preset 3), n_ctx {N_CTX}; {N} utterances, {SLOTS} slots, "
            f"budgets {min(budgets)}..{max(budgets)} (sum {live}), prompt tokens {sum(len(p) for p in prompts)}")
        say(f"queue:  steps {stats['steps']}, refills {stats['refills']}, prefill chunks {stats['prefill_chunks']}, "
            f"occupancy {stats['live_slot_steps'] / (stats['steps'] * SLOTS):.3f}")
        say(f"groups: steps {gsteps}, occupancy {live / (gsteps * SLOTS):.3f}")
        ratios, digest = [], hashlib.sha256()
        for i in range(PAIRS):
            if i % 2 == 0:
                (q, tq, _), (g, tg) = queue(), groups()
            else:
                (g, tg), (q, tq, _) = groups(), queue()
            for t in tq + tg:
                digest.update(np.asarray(t, np.int32).tobytes())
            ratios.append(g / q)
            say(f"pair {i}: queue {q * 1e3:.1f} ms, groups {g * 1e3:.1f} ms, groups / queue {g / q:.3f}")
        say(f"median groups / queue: {float(np.median(ratios)):.3f} (min {min(ratios):.3f}, max {max(ratios):.3f})")
        say(f"tokens sha256: {digest.hexdigest()}")
        llm.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
