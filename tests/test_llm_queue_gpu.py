"""GPU parity: the utterance queue on the batched decode (mio_hip_llm_generate_queue,
csrc/host/llm_batch.cpp + k_bt_refill / k_bt_admit in csrc/hip/llm_prefill.hip) vs the
single-utterance decode (mio_hip_llm_generate).

N utterances run on `slots` streams; a slot whose utterance has ended is prefilled with the next
one between two step graphs while the other slots keep decoding. Like a stream of
mio_hip_llm_generate_batch (test_llm_batch_gpu.py), every utterance's per-token arithmetic and
sampler noise are the single-stream decode's, so its tokens equal generate(prompt_u, seed_u)
EXACTLY, whatever slot it ran on, whatever ran there before and whatever its neighbours do.
"""
import os
import subprocess
import wave

import numpy as np
import pytest

import miotts_amd as m

pytestmark = pytest.mark.gpu

ALLOW = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "miotts-llama.cpp_amd", "build")


@pytest.fixture(scope="module")
def llm_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("llm_queue")
    return {p: m.synth_llm(str(d / f"llm{p}.gguf"), p, 1) for p in (0, 1)}


def _prompts(N, seed, lo=3, hi=40):
    rng = np.random.default_rng(seed)
    # ragged lengths, including a 1-token prompt (nothing to prefill for that utterance)
    lens = [1 if u == 1 else int(rng.integers(lo, hi)) for u in range(N)]
    return [list(rng.integers(0, 256, n)) for n in lens]


def _assert_equals_single(g, prompts, got, n, T, seeds, **kw):
    refs = [g.generate(p, n, T, s, **kw) for p, s in zip(prompts, seeds)]
    for u, (a, r) in enumerate(zip(got, refs)):
        assert np.array_equal(a, r), (u, a, r)
    return refs


# EOS_K: the sampling window of test 1 is [SYNTH_EOT, SYNTH_SPEECH0 + EOS_K), one end token among
# EOS_K + 1 ids at temperature 2.0 (test_batch_stops_at_eos's window, wider: utterances of a few
# step graphs instead of a few steps)
EOS_K = 20


@pytest.mark.parametrize("preset", [0, 1])
def test_queue_equals_single_ragged_by_end_tokens(device, llm_files, preset):
    """12 utterances on 3 slots, ended by the end tokens they sample: every one equals its
    single-stream generate, and 9 of them started in a slot another one had used."""
    g = m.Llm(device, llm_files[preset], 256)
    prompts = _prompts(12, 50 + preset)
    seeds = [300 + 7 * u for u in range(12)]
    kw = dict(allow=(m.SYNTH_EOT, m.SYNTH_SPEECH0 + EOS_K), eos=(m.SYNTH_EOT, m.SYNTH_IM_END))
    refs = [g.generate(p, 120, 2.0, s, **kw) for p, s in zip(prompts, seeds)]
    lens = [len(r) for r in refs]
    print("single-stream lengths", lens)
    # precondition: the single-stream lengths are ragged and end tokens do end utterances
    assert len(set(lens)) > 1 and min(lens) < 120, lens
    got, stats = g.generate_queue(prompts, 120, 2.0, seeds, slots=3, **kw)
    print(stats)
    for u in range(12):
        assert np.array_equal(got[u], refs[u]), (u, got[u], refs[u])
        assert (got[u] != m.SYNTH_EOT).all()
    assert stats["refills"] == 9
    g.close()


def test_queue_one_slot_with_end_tokens(device, llm_files):
    """One slot, utterances ended by end tokens: the host learns of every end from the mapped word
    alone, one utterance at a time, and must go on to the next utterance each time (a loop that
    ended on 'every slot is finished' with utterances waiting would return them empty)."""
    g = m.Llm(device, llm_files[0], 256)
    prompts = _prompts(8, 61, 3, 20)
    seeds = [500 + u for u in range(8)]
    kw = dict(allow=(m.SYNTH_EOT, m.SYNTH_SPEECH0 + EOS_K), eos=(m.SYNTH_EOT, m.SYNTH_IM_END))
    refs = [g.generate(p, 120, 2.0, s, **kw) for p, s in zip(prompts, seeds)]
    assert min(len(r) for r in refs) < 120
    got, stats = g.generate_queue(prompts, 120, 2.0, seeds, slots=1, **kw)
    for u in range(8):
        assert np.array_equal(got[u], refs[u]), (u, got[u], refs[u])
    assert stats["slot_of"] == [0] * 8 and stats["refills"] == 7
    st = stats["start_step"]
    # end token included, every utterance sampled len + 1 steps (or its 120) before the next began
    assert all(st[u + 1] >= st[u] + min(len(refs[u]) + 1, 120) for u in range(7)), st
    g.close()


def _schedule(budgets, slots, gs):
    """The host loop's rule, restated: at every boundary the finished slots (empty, or budget
    issued) take the next utterances in slot order; then min(gs, longest remaining budget) steps."""
    N, S = len(budgets), min(slots, len(budgets))
    cur, start, steps, nxt = [-1] * S, [0] * S, 0, 0
    slot_of, start_step = [-1] * N, [-1] * N
    while True:
        for b in range(S):
            if nxt < N and (cur[b] < 0 or steps - start[b] >= budgets[cur[b]]):
                cur[b], start[b], slot_of[nxt], start_step[nxt] = nxt, steps, b, steps
                nxt += 1
        left = max(budgets[cur[b]] - (steps - start[b]) for b in range(S))
        if left <= 0:
            return steps, slot_of, start_step
        steps += min(gs, left)


def test_queue_ragged_by_context_budget_and_step_count(device, llm_files):
    """n_ctx 128, no end tokens: a prompt of 120 tokens has a budget of 128 - 120 + 1 = 9 tokens,
    one of 8 tokens the whole max_tokens = 120. Budgets [120, 9, 9] x 4 on 3 slots: groups of 3
    in order would take 4 x 120 = 480 steps, no schedule fewer than ceil(552 / 3) = 184. The host
    decides a spent budget from its own counters, so steps, slot_of and start_step are a function
    of the budgets and the steps per graph alone (_schedule).
    Measured (8 steps per graph, the default): 256 steps."""
    g = m.Llm(device, llm_files[0], 128)
    rng = np.random.default_rng(9)
    plens = [8, 120, 120] * 4
    budgets = [120, 9, 9] * 4
    prompts = [list(rng.integers(0, 256, n)) for n in plens]
    seeds = [40 + u for u in range(12)]
    got, stats = g.generate_queue(prompts, 120, 0.8, seeds, slots=3, allow=ALLOW)
    print(stats)
    _assert_equals_single(g, prompts, got, 120, 0.8, seeds, allow=ALLOW)
    assert [len(t) for t in got] == budgets
    assert stats["live_slot_steps"] == sum(budgets) == 552
    assert 184 <= stats["steps"] < 480, stats
    steps, slot_of, start_step = _schedule(budgets, 3, m.llm_graph_steps())
    assert (stats["steps"], stats["slot_of"], stats["start_step"]) == (steps, slot_of, start_step), stats
    # whatever the rule: admission in index order, and no two utterances on a slot at once
    st = stats["start_step"]
    assert all(st[u] <= st[u + 1] for u in range(11)), st
    for b in range(3):
        on = [u for u in range(12) if stats["slot_of"][u] == b]
        assert on == sorted(on)
        for a, c in zip(on, on[1:]):
            assert st[c] >= st[a] + len(got[a]), (b, a, c, st)
    assert sorted(set(stats["slot_of"])) == [0, 1, 2]
    g.close()


def test_queue_lfm2_slot_reuse(device, synth_llm_path):
    """lfm2 (preset 7: short-conv layers with a per-stream ring of B*X rows): 6 utterances on 2
    slots, each equal to its single-stream generate: an utterance must not see the ring rows the
    slot's previous utterance left."""
    g = m.Llm(device, synth_llm_path(7), 256)
    prompts = _prompts(6, 77, 2, 12)
    seeds = [900 + 3 * u for u in range(6)]
    got, stats = g.generate_queue(prompts, 24, 0.8, seeds, slots=2, allow=ALLOW)
    _assert_equals_single(g, prompts, got, 24, 0.8, seeds, allow=ALLOW)
    assert stats["refills"] == 4 and all(len(t) == 24 for t in got)
    g.close()


def test_queue_sampler_chain_history_is_per_utterance(device, llm_files):
    """top-k 20 + repeat penalty 1.3: the penalty history is the utterance's own sampled tokens
    (first_step = its P), not what the slot's previous utterance sampled."""
    g = m.Llm(device, llm_files[0], 256)
    g.set_sampling(top_k=20, repeat_penalty=1.3)
    prompts = _prompts(6, 31, 3, 20)
    seeds = [11 + u for u in range(6)]
    # a narrow window: tokens repeat, so the penalties act
    allow = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 64)
    got, stats = g.generate_queue(prompts, 24, 0.8, seeds, slots=2, allow=allow)
    _assert_equals_single(g, prompts, got, 24, 0.8, seeds, allow=allow)
    assert stats["refills"] == 4
    g.set_sampling()
    g.close()


def test_queue_edges(device, llm_files):
    g = m.Llm(device, llm_files[0], 256)
    prompts = _prompts(20, 5)
    seeds = [700 + u for u in range(20)]
    refs = [g.generate(p, 16, 0.8, s, allow=ALLOW) for p, s in zip(prompts, seeds)]
    # N = 1 and N < slots: the generate_batch of the same prompts
    for N in (1, 5):
        got, stats = g.generate_queue(prompts[:N], 16, 0.8, seeds[:N], slots=8, allow=ALLOW)
        bat = g.generate_batch(prompts[:N], 16, 0.8, seeds[:N], allow=ALLOW)
        assert all(np.array_equal(a, b) for a, b in zip(got, bat)) and len(got) == N
        assert all(np.array_equal(a, r) for a, r in zip(got, refs))
        assert stats["refills"] == 0 and stats["slot_of"] == list(range(N))
    # one slot: N single generates one after another
    got, stats = g.generate_queue(prompts[:4], 16, 0.8, seeds[:4], slots=1, allow=ALLOW)
    assert all(np.array_equal(a, r) for a, r in zip(got, refs))
    assert stats["slot_of"] == [0] * 4 and stats["refills"] == 3 and stats["steps"] == 64
    # 16 slots, 20 utterances
    got, stats = g.generate_queue(prompts, 16, 0.8, seeds, slots=16, allow=ALLOW)
    for u in range(20):
        assert np.array_equal(got[u], refs[u]), u
    assert stats["refills"] == 4 and stats["live_slot_steps"] == 20 * 16
    # a batch after a queue call on the same handle: nothing of the slots' state leaks
    bat = g.generate_batch(prompts[3:9], 16, 0.8, seeds[3:9], allow=ALLOW)
    assert all(np.array_equal(a, r) for a, r in zip(bat, refs[3:9]))
    g.close()


def test_queue_rejects_bad_arguments(device, llm_files):
    g = m.Llm(device, llm_files[0], 64)
    p = [[256, 257, 65]] * 6
    for slots in (0, 17):
        with pytest.raises(m.HipError):
            g.generate_queue(p, 4, 0.8, slots=slots)
    bad = list(p)
    bad[5] = [256] * 65  # longer than n_ctx 64: refused before anything is queued
    with pytest.raises(m.HipError):
        g.generate_queue(bad, 4, 0.8, slots=2)
    with pytest.raises(m.HipError):
        g.generate_queue([[256, 257], [256, 10 ** 6]], 4, 0.8, slots=2)  # out of vocabulary
    got = g.generate_batch(p[:2], 8, 0.8, [5, 6], allow=ALLOW)
    for b in range(2):
        assert np.array_equal(got[b], g.generate(p[b], 8, 0.8, 5 + b, allow=ALLOW))
    g.close()


def _run(args, timeout=300):
    p = subprocess.run([os.path.join(BIN, "miotts")] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"miotts rc={p.returncode}\n{p.stdout}\n{p.stderr[-2000:]}"
    assert "batched decode unavailable" not in p.stderr, p.stderr[-2000:]


def test_miotts_batch_of_20_lines(tmp_path):
    """`miotts --batch` with more lines than the engine has slots: 20 files, and the ones spot-checked
    (the first, one of the first 16 and one admitted into a used slot) have the bytes a single
    `miotts -p LINE` run writes."""
    d = tmp_path
    files = {"llm": m.synth_llm(str(d / "llm1.gguf"), 1, 1), "codec": m.synth_codec(str(d / "codec.gguf"), 1, 1),
             "voice": m.synth_voice(str(d / "voice.emb.gguf"), 7)}
    words = ["テスト", "こんにちは", "今日はいい天気ですね", "はい", "ありがとうございます"]
    lines = ["、".join(words[(i + j) % 5] for j in range(1 + i % 4)) + "。" for i in range(20)]
    (d / "batch.txt").write_text("\n".join(lines) + "\n", "utf-8")
    common = ["-m", files["llm"], "-c", files["codec"], "-v", files["voice"], "--max-tokens", 24, "--speech-only",
              "--ignore-eos"]
    _run(common + ["--batch", d / "batch.txt", "-o", d / "b.wav"])
    for i in range(20):
        with wave.open(str(d / f"b_{i:03d}.wav")) as w:
            assert w.getnframes() > 0, i
    for i in (0, 9, 18):
        _run(common + ["-p", lines[i], "-o", d / f"s{i}.wav"])
        assert (d / f"b_{i:03d}.wav").read_bytes() == (d / f"s{i}.wav").read_bytes(), i
