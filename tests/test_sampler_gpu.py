"""GPU parity of the on-device sampler on the GPU's own logits, against tests/np_sampler.py.

Replay scheme: after a generate of n tokens from a prompt of P + 1 tokens, prompt + tokens[:-1]
is decoded teacher-forced with eval from position 0; the logits at position P + i are what step
P + i sampled from (the suite pins the batched prefill and the batched decode to the single-token
step bit for bit, test_llm_gpu.py / test_llm_batch_gpu.py). logits() right after the generate
must equal the last replayed row bit for bit, which ties the replay to the run. Token i must then
be np_sampler.sample(logits, T, seed, P + i, lo, hi) under np_sampler's near-tie rule; near-ties
are counted per case (a temperature and window kind over its prompts and seeds) and capped at 1 %
of the case's steps; a case that asserts an exact id contains none.

Covered: the noise hash and its counters (64-bit seeds, step = n_prompt - 1 + i after a batched
prefill, after a prefill of more than one chunk and after forced steps), the [lo, hi) clipping at
both ends, the empty window, allow_hi past n_vocab, ties -> lowest id through the partial
producers k_lm_head, k_bt_lm_head (MIO_BT_LM_MMQ=0), k_bt_gumbel and the reducers (k_sample, the
layer-0 attn_in, k_bt_sample), v / T at extreme temperatures, k_lm_head's second row register
(MIO_LM_WGM=1 on the 1.7B shape), and the largest draw of the noise hash (finite since the clamp
in gumbel()). The teeth of these cases are in test_sampler_ref.py.
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import miotts_amd as m
import np_sampler as S
from miotts_amd import gguf_np

pytestmark = pytest.mark.gpu

N_CTX = 256
N_TOK = 96  # several 8-step graphs and the flush sampler
HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _replay(g, prompt, toks):
    """Logits rows of positions P .. P + len(toks) - 1 of prompt + toks[:-1], by eval from 0."""
    seq = [int(t) for t in prompt] + [int(t) for t in toks[:-1]]
    P = len(prompt) - 1
    rows = []
    for pos, t in enumerate(seq):
        lg = g.eval(t, pos)
        if pos >= P:
            rows.append(lg)
    return rows


def _run(g, prompt, n, T, seed, allow):
    """One generate + replay: (tokens, replayed rows, rejected steps, near-ties)."""
    toks = g.generate(prompt, n, T, seed, allow=allow)
    last = g.logits()
    assert len(toks) == n
    rows = _replay(g, prompt, toks)
    assert np.array_equal(_bits(last), _bits(rows[-1])), "replay does not reproduce the run's last logits"
    lo, hi = S.window(allow, g.n_vocab)
    bad, near = S.compare(toks, rows, T, seed, len(prompt) - 1, lo, hi)
    return toks, rows, bad, near


class _Tally:
    """Near-ties and steps per case; the cap is asserted at the end."""

    def __init__(self):
        self.c = {}

    def add(self, case, near, steps):
        a = self.c.setdefault(case, [0, 0])
        a[0] += near
        a[1] += steps

    def check(self):
        print("near-ties per case (near, steps):", self.c)
        over = {k: v for k, v in self.c.items() if v[0] > S.CAP * v[1]}
        assert not over, over


def _tie_file(src, dst):
    """Copy of src whose token_embd.weight rows [TIE_A, TIE_A + TIE_N) are row TIE_A's bytes (a tied
    embedding: the same rows of the output matrix)."""
    assert S.TIE_A % 26 not in (0, 25)  # the block starts inside a wave of a 26-row workgroup
    shutil.copyfile(src, dst)
    r = gguf_np.GGUFReader(dst)
    assert "output.weight" not in r.by_name
    t = r.tensor("token_embd.weight")
    n_embd, n_vocab = t.ne
    rb = t.nbytes // n_vocab
    start = r.data_offset + t.offset
    del r
    mm = np.memmap(dst, dtype=np.uint8, mode="r+")
    row = np.array(mm[start + S.TIE_A * rb:start + (S.TIE_A + 1) * rb])
    for i in range(S.TIE_A, S.TIE_A + S.TIE_N):
        mm[start + i * rb:start + (i + 1) * rb] = row
    mm.flush()
    del mm
    return dst


@pytest.fixture(scope="module")
def tie_path(synth_llm_path, tmp_path_factory):
    return _tie_file(synth_llm_path(0), str(tmp_path_factory.mktemp("sampler") / "tie.gguf"))


@pytest.mark.parametrize("preset", [0, 1, 11])
def test_wide_windows(device, synth_llm_path, preset):
    """T 0.8, 5 and 0.05 over the speech window, T 0.05 over the whole vocabulary, a clipped
    allow_hi: every prompt length, the seeds rotated so that each (prompt, seed) pair occurs."""
    g = m.Llm(device, synth_llm_path(preset), N_CTX)
    tally = _Tally()
    for ci, (name, T, allow) in enumerate(S.wide_cases(g.n_vocab)):
        for pi, plen in enumerate(S.PROMPT_LENS):
            seed = S.SEEDS[(ci + pi) % 3]
            toks, _, bad, near = _run(g, S.prompt(plen), N_TOK, T, seed, allow)
            assert not bad, (name, plen, seed, bad[:3])
            tally.add(name, near, len(toks))
            lo, hi = S.window(allow, g.n_vocab)
            assert ((toks >= lo) & (toks < hi)).all()
    tally.check()
    g.close()


@pytest.mark.parametrize("preset", [0, 1, 11])
def test_narrow_windows(device, synth_llm_path, preset):
    """Windows of width 1, 2, 3, 63, 64, 65 and 129 at offset 0, at n_vocab - width and at three
    random offsets, at T 0.8 and greedy; prompts and seeds rotate."""
    g = m.Llm(device, synth_llm_path(preset), N_CTX)
    tally = _Tally()
    for wi, (lo, hi) in enumerate(S.narrow_windows(g.n_vocab)):
        for T in (0.8, 0.0):
            plen, seed = S.PROMPT_LENS[wi % 3], S.SEEDS[(wi // 3) % 3]
            toks, _, bad, near = _run(g, S.prompt(plen), N_TOK if plen < 100 else 24, T, seed, (lo, hi))
            assert not bad, (lo, hi, T, plen, seed, bad[:3])
            tally.add(f"T{T} width {hi - lo}", near, len(toks))
            assert ((toks >= lo) & (toks < hi)).all()
            if hi - lo == 1 or T == 0.0:
                assert near == 0
            if hi - lo == 1:
                assert (toks == lo).all()
    tally.check()
    g.close()


@pytest.mark.parametrize("preset", [0, 1, 11])
def test_exact_edges(device, synth_llm_path, preset):
    """The empty window returns lo. At T = 1e-30 the quotient v / T (about 1e30 v, finite in f32)
    absorbs the noise and the largest logit wins. At T = 1e-45, a subnormal f32, the quotient
    overflows: every positive logit ties at +inf and the token is the lowest id of the window with
    a positive logit. Both are exact."""
    g = m.Llm(device, synth_llm_path(preset), N_CTX)
    p = S.prompt(5)
    for T in (0.0, 0.8):
        for lo in (0, 777, g.n_vocab - 1):
            assert (g.generate(p, 12, T, 42, allow=(lo, lo)) == lo).all(), (T, lo)
    for allow in (S.SPEECH, (-1, -1), (5000, 5065)):
        lo, hi = S.window(allow, g.n_vocab)
        toks, rows, bad, near = _run(g, p, 24, 1e-30, 679, allow)
        want = [lo + int(np.argmax(r[lo:hi])) for r in rows]
        assert toks.tolist() == want and not bad and near == 0, (allow, toks, want)
        toks, rows, bad, near = _run(g, p, 24, 1e-45, 679, allow)
        want = [lo + int(np.argmax(r[lo:hi] > 0)) for r in rows]
        assert all((r[lo:hi] > 0).any() for r in rows)
        assert toks.tolist() == want and not bad and near == 0, (allow, toks, want)
    g.close()


def test_ties_single_stream(device, tie_path):
    """700 bit-equal logits: inside the block greedy returns lo through k_lm_head's partials and
    both reducers (8-step graphs: the layer-0 attn_in; the last token: k_sample), and T > 0 returns
    the argmax of the noise alone."""
    g = m.Llm(device, tie_path, N_CTX)
    blk = slice(S.TIE_A, S.TIE_A + S.TIE_N)
    tally = _Tally()
    for wi, (lo, hi) in enumerate(S.tie_windows()):
        plen, seed = S.PROMPT_LENS[wi % 2], S.SEEDS[wi % 3]
        p = S.prompt(plen)
        toks, rows, bad, near = _run(g, p, 20, 0.0, seed, (lo, hi))
        assert all((_bits(r[blk]) == _bits(r[blk])[0]).all() for r in rows), "tied rows give unequal logits"
        assert (toks == lo).all() and not bad and near == 0, (lo, hi, toks)
        toks, rows, bad, near = _run(g, p, 20, 0.8, seed, (lo, hi))
        ids = np.arange(lo, hi)
        want = [lo + int(np.argmax(S.noise(seed, len(p) - 1 + i, ids))) for i in range(len(toks))]
        assert all((_bits(r[blk]) == _bits(r[blk])[0]).all() for r in rows)
        assert toks.tolist() == want and not bad and near == 0, (lo, hi, toks, want)
        tally.add("tie", near, 2 * len(toks))
    # a window wider than the block at T = 0: the block's logit wins or loses as a whole, the
    # winner is the reference's
    toks, rows, bad, near = _run(g, S.prompt(5), 20, 0.0, 42, (S.TIE_A - 100, S.TIE_A + S.TIE_N + 100))
    assert not bad and near == 0
    tally.check()
    g.close()


def _check_batch(g, case, got, tally):
    lo, hi = S.window(case["allow"], g.n_vocab)
    for b, (p, seed) in enumerate(zip(case["prompts"], case["seeds"])):
        toks = np.asarray(got[b], np.int32)
        assert len(toks) == S.BATCH_TOKENS
        rows = _replay(g, p, toks)
        bad, near = S.compare(toks, rows, case["T"], seed, len(p) - 1, lo, hi)
        assert not bad, (case["name"], b, bad[:3])
        tally.add(case["name"], near, len(toks))
        if case["name"].endswith("tie T0"):
            assert (toks == lo).all() and near == 0, (case["name"], b, toks)
        if case["name"].endswith("tie T0.8"):
            want = [lo + int(np.argmax(S.noise(seed, len(p) - 1 + i, np.arange(lo, hi)))) for i in range(len(toks))]
            assert toks.tolist() == want and near == 0, (case["name"], b, toks, want)
        if case["T"] == 0.0:
            assert near == 0


def test_batch_default_engine(device, synth_llm_path, tie_path):
    """generate_batch (logits on the matrix cores, partials by k_bt_gumbel, k_bt_sample): every
    stream against numpy on its own replayed logits."""
    gs = {False: m.Llm(device, synth_llm_path(0), N_CTX), True: m.Llm(device, tie_path, N_CTX)}
    tally = _Tally()
    for case in S.batch_cases(gs[False].n_vocab):
        g = gs[case["tie"]]
        got = g.generate_batch(case["prompts"], S.BATCH_TOKENS, case["T"], case["seeds"], allow=case["allow"])
        _check_batch(g, case, got, tally)
    tally.check()
    for g in gs.values():
        g.close()


_BATCH_SCRIPT = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import miotts_amd as m
import np_sampler as S
dev = m.Device(0)
gs = {False: m.Llm(dev, sys.argv[3], 256), True: m.Llm(dev, sys.argv[4], 256)}
out = []
for case in S.batch_cases(gs[False].n_vocab):
    got = gs[case["tie"]].generate_batch(case["prompts"], S.BATCH_TOKENS, case["T"], case["seeds"], allow=case["allow"])
    out.append([[int(t) for t in s] for s in got])
print(json.dumps(out))
"""


def _child(script_path, args, env):
    pkg = os.path.dirname(os.path.dirname(m.__file__))
    p = subprocess.run([sys.executable, str(script_path), pkg, HERE] + args, capture_output=True, text=True,
                       timeout=240, env=dict(os.environ, **env))
    assert p.returncode == 0, (env, p.stderr[-2000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_batch_dot_engine(device, synth_llm_path, tie_path, tmp_path):
    """The same cases with MIO_BT_LM_MMQ=0 (k_bt_lm_head: logits and partials in one launch), run in
    a fresh process (the switch is read once); the tokens are checked here on this process's
    single-stream replay."""
    script = tmp_path / "batch.py"
    script.write_text(_BATCH_SCRIPT)
    outs = _child(script, [synth_llm_path(0), tie_path], {"MIO_BT_LM_MMQ": "0"})
    gs = {False: m.Llm(device, synth_llm_path(0), N_CTX), True: m.Llm(device, tie_path, N_CTX)}
    tally = _Tally()
    cases = S.batch_cases(gs[False].n_vocab)
    assert len(outs) == len(cases)
    for case, got in zip(cases, outs):
        _check_batch(gs[case["tie"]], case, got, tally)
    tally.check()
    for g in gs.values():
        g.close()


_R1_SCRIPT = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import miotts_amd as m
import np_sampler as S
dev = m.Device(0)
g = m.Llm(dev, sys.argv[3], 256)
p = S.prompt(5)
toks = g.generate(p, 24, 0.8, 42, allow=S.SPEECH)
last = g.logits()
rows = []
for pos, t in enumerate(p + [int(t) for t in toks[:-1]]):
    lg = g.eval(t, pos)
    if pos >= len(p) - 1:
        rows.append(lg)
bad, near = S.compare(toks, rows, 0.8, 42, len(p) - 1, *S.SPEECH)
print(json.dumps(dict(tokens=[int(t) for t in toks], cu=dev.cu_count(), n_vocab=g.n_vocab, near=int(near),
                      bad=[(i, t, tuple(float(x) for x in pk)) for i, t, pk in bad],
                      tied=bool(np.array_equal(last.view(np.uint32), rows[-1].view(np.uint32))))))
"""


def test_second_row_register(device, synth_llm_path, tmp_path):
    """k_lm_head's second row register (rows 64..127 of a wave) is live only when a wave owns more
    than 64 rows: the 1.7B vocabulary with one lm_head workgroup per CU (MIO_LM_WGM=1, a fresh
    process). 24 tokens in parity with numpy on the replayed logits, and equal to the default
    configuration's."""
    script = tmp_path / "r1.py"
    script.write_text(_R1_SCRIPT)
    path = synth_llm_path(3)
    r = _child(script, [path], {"MIO_LM_WGM": "1"})
    assert r["n_vocab"] / (r["cu"] * 8) > 64, r
    assert r["tied"] and not r["bad"] and r["near"] == 0, r
    g = m.Llm(device, path, N_CTX)
    toks, _, bad, near = _run(g, S.prompt(5), 24, 0.8, 42, S.SPEECH)
    g.close()
    assert not bad and toks.tolist() == r["tokens"], (toks, r["tokens"])


def test_largest_draw_is_finite(device, synth_llm_path):
    """(seed 679, step 6, id 4872) draws h >> 40 == 2^24 - 1: before the clamp in gumbel() its noise
    was +inf and id 4872 won whatever its logit (observed on the build before the fix: token 2 ==
    4872). With finite noise token 2 is the reference's."""
    g = m.Llm(device, synth_llm_path(0), N_CTX)
    p = S.prompt(5)
    assert int(S.draw(679, 6, [4872])[0]) == (1 << 24) - 1 and len(p) - 1 + 2 == 6
    toks, rows, bad, near = _run(g, p, 4, 0.05, 679, S.SPEECH)
    lo, hi = S.SPEECH
    assert lo + int(np.argmax(rows[2][lo:hi])) != 4872, "id 4872 has the window's largest logit: the case lost its meaning"
    pick = S.sample(rows[2], 0.05, 679, 6, lo, hi)
    print("tokens", toks.tolist(), "reference at step 6:", pick)
    assert not pick.near_tie and int(toks[2]) == pick.winner, (toks, pick)
    assert not bad and near == 0
    g.close()
