"""GPU: all-BF16 lfm2 files (three of the six published sizes are LFM2 hybrids, every size ships
in BF16) on the multi-token engine: the chunked prompt prefill and the batched decode.

In a short-conv layer the engine runs in_proj on k_pf_attn_in<NP, 30, 30> (the B | C rows as q,
the X rows as v, token stride 3 n_embd), k_bt_conv writing bf16 records (laid out for 2 n_embd),
k_bt_conv_state, and out_proj on k_pf_attn_out<NP, 30>. A row's value depends on the lane order
within the row and the row-total tree alone, both shared with the decode step, and the conv record
comes from the decode step's conv_load / conv_quant: so every comparison between the two engines
here is bit for bit, with no tolerance.

Models:
  T  synth_llm_as(7, 30): n_embd 256, 5 layers, short conv at 0, 2, 3, attention at 1, 4.
  M  synth_llm_shape(7, 30, n_embd 1024, 4 layers, 16 / 8 heads, n_ff 2048), about 110 MB. At
     n_embd 256 a 128-token chunk of bf16 records (0.7 KB per token) fits LDS and the launches
     never split; at 1024 the records are over 2 KB per token, 256 KB per chunk against 160 KB,
     so the conv launches run in token sub-ranges and the stride of pb.qkv in them is exercised.

The conv rings are compared in every slot but n & 3: a chunk of the batched prefill stores the
rows of its last two positions only (nothing reads older ones), so after n positions the slot
that position n overwrites before anything reads it holds position n - 4 after a token-by-token
decode and an older row (or nothing) after the prefill. The three other slots hold positions
n - 3 .. n - 1 on both paths.

The last test is a yardstick for the single-stream decode of T against the oracle. On the parent
commit it fails (measured there: per-position max-rel up to 1.42, median 0.96, all 150 positions
over the 5e-2 bound, argmax agreement 73 / 150 against 95 %): qmat_rows had no BF16 case, so the
decode step read the X rows of in_proj from the B rows. With the row offset in place the decode
step meets test_lfm2_gpu.py's bounds (max-rel 5.6e-3, argmax 150 / 150).
"""
import os
import subprocess

import numpy as np
import pytest

import miotts_amd as m
import pyoracle

pytestmark = pytest.mark.gpu

ALLOW = (m.SYNTH_SPEECH0, m.SYNTH_SPEECH0 + 12800)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "miotts-llama.cpp_amd", "build")
CHUNK = 128  # kPrefillB


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lfm2_bf16")
    return {"T": m.synth_llm_as(str(d / "t.gguf"), 7, 30, 1),
            "M": m.synth_llm_shape(str(d / "m.gguf"), 7, 30, 1, n_embd=1024, n_layer=4, n_head=16, n_head_kv=8,
                                   n_ff=2048),
            "codec_tiny": m.synth_codec(str(d / "codec_tiny.gguf"), 1, 1),
            "voice": m.synth_voice(str(d / "voice.emb.gguf"), 7),
            "dir": d}


def _conv_layers(g):
    """(short-conv layers, attention layers): the ring getter refuses an attention layer."""
    conv, att = [], []
    for il in range(g.n_layer):
        try:
            g.conv_ring(il)
            conv.append(il)
        except m.HipError:
            att.append(il)
    return conv, att


def _state(g, conv, att, n):
    rings = {il: g.conv_ring(il).view(np.uint32).copy() for il in conv}
    kv = {il: tuple(a.view(np.uint16).copy() for a in g.kv_rows(il, n)) for il in att}
    return rings, kv


@pytest.mark.parametrize("model,n", [("T", 2), ("T", 3), ("T", 17), ("T", 131), ("T", 150), ("T", 257), ("M", 131)])
def test_prefill_equals_sequential(device, files, model, n):
    """The chunked prefill leaves the logits, the conv rings and the K/V rows of a token-by-token
    decode, bit for bit. n = 2, 3: the conv window reaches before the sequence start; 131: positions
    128-130 take window rows from the ring the previous chunk left; 257: two hand-offs. It spends
    ceil((n - 1) / 128) weight passes on the prompt (the forced-step prefill spends n - 1)."""
    g = m.Llm(device, files[model], 384)
    conv, att = _conv_layers(g)
    assert (conv, att) == (([0, 2, 3], [1, 4]) if model == "T" else ([0, 2, 3], [1]))
    toks = np.random.default_rng(500 + n).integers(0, g.n_vocab, n)
    batched = g.prefill(toks)
    chunks = g.prompt_chunks()
    rb, kb = _state(g, conv, att, n)
    seq = None
    for pos, t in enumerate(toks):
        seq = g.eval(int(t), pos)
    rs, ks = _state(g, conv, att, n)
    print(f"{model} n={n}: prompt_chunks {chunks}, max |logit diff| {float(np.abs(batched - seq).max()):.3g}")
    assert np.array_equal(batched.view(np.uint32), seq.view(np.uint32)), float(np.abs(batched - seq).max())
    live = [s for s in range(4) if s != (n & 3)]
    for il in conv:
        assert np.array_equal(rb[il][live], rs[il][live]), ("ring", il)
    for il in att:
        assert np.array_equal(kb[il][0], ks[il][0]) and np.array_equal(kb[il][1], ks[il][1]), ("kv", il)
    assert chunks == (n - 1 + CHUNK - 1) // CHUNK, chunks
    g.close()


def _prompts(B, seed, lo=3, hi=40):
    rng = np.random.default_rng(seed)
    lens = [1 if b == 1 else int(rng.integers(lo, hi)) for b in range(B)]
    return [list(rng.integers(0, 256, n)) for n in lens]


@pytest.mark.parametrize("model,B,ntok", [("T", 3, 24), ("T", 12, 24), ("T", 16, 24), ("M", 4, 16)])
def test_batch_equals_single_streams(device, files, model, B, ntok):
    """B ragged utterances (stream 1 a 1-token prompt) decoded together equal their single-stream
    decodes exactly; at B = 12 the prompts go up to 60 tokens, so the flattened prefill splits a
    stream across two chunks."""
    g = m.Llm(device, files[model], 256)
    prompts = _prompts(B, 70 + B, 3, 40 if B < 10 else 60)
    seeds = [1000 + 17 * b for b in range(B)]
    got = g.generate_batch(prompts, ntok, 0.8, seeds, allow=ALLOW)
    for b in range(B):
        ref = g.generate(prompts[b], ntok, 0.8, seeds[b], allow=ALLOW)
        assert g.prompt_chunks() == (len(prompts[b]) - 1 + CHUNK - 1) // CHUNK
        assert len(ref) == ntok and np.array_equal(got[b], ref), (b, got[b], ref)
    g.close()


def test_batch_streams_end_at_different_steps(device, files):
    """A narrow window around the end token at temperature 2: the streams end at different steps,
    and a frozen stream does not disturb the rings of the live ones."""
    g = m.Llm(device, files["T"], 256)
    prompts = [[256, 257, 65, 258, 257], [256, 257, 66, 67, 258, 257], [256, 257, 68, 258, 257]]
    allow = (m.SYNTH_EOT, m.SYNTH_SPEECH0 + 3)
    eos = (m.SYNTH_EOT, m.SYNTH_IM_END)
    got = g.generate_batch(prompts, 200, 2.0, [7, 8, 9], allow=allow, eos=eos, check_interval=20)
    for b, p in enumerate(prompts):
        ref = g.generate(p, 200, 2.0, 7 + b, allow=allow, eos=eos, check_interval=20)
        assert np.array_equal(got[b], ref), (b, got[b], ref)
        assert len(got[b]) < 200 and (got[b] != m.SYNTH_EOT).all()
    print("stream lengths", [len(x) for x in got])
    assert len({len(x) for x in got}) > 1
    g.close()


def test_batch_with_sampler_chain(device, files):
    """The sampler chain on (the graph pair with the chain launch): batch == single."""
    g = m.Llm(device, files["T"], 256)
    g.set_sampling(top_k=40, repeat_penalty=1.1)
    prompts = _prompts(3, 91)
    seeds = [5, 6, 7]
    got = g.generate_batch(prompts, 24, 0.8, seeds, allow=ALLOW)
    for b in range(3):
        ref = g.generate(prompts[b], 24, 0.8, seeds[b], allow=ALLOW)
        assert np.array_equal(got[b], ref), (b, got[b], ref)
    g.close()


def run(args, timeout=300):
    p = subprocess.run([os.path.join(BIN, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"{args[0]} rc={p.returncode}\n{p.stdout}\n{p.stderr[-2000:]}"
    return p.stderr


def test_miotts_batch_cli(files):
    """`miotts --batch` on T: the lines decode on the batched engine (no one-at-a-time fallback)
    and each OUT_nnn.wav has the bytes of the single `-p` run."""
    d = files["dir"]
    prompts = ["テストです。", "こんにちは。", "今日はいい天気ですね。"]
    (d / "batch.txt").write_text("\n".join(prompts) + "\n", "utf-8")
    common = ["-m", files["T"], "-c", files["codec_tiny"], "-v", files["voice"], "--max-tokens", 40, "--speech-only",
              "--ignore-eos"]
    err = run(["miotts"] + common + ["--batch", d / "batch.txt", "-o", d / "b.wav"])
    assert "batched decode unavailable" not in err, err[-2000:]
    for i, p in enumerate(prompts):
        run(["miotts"] + common + ["-p", p, "-o", d / f"s{i}.wav"])
        assert (d / f"b_{i:03d}.wav").read_bytes() == (d / f"s{i}.wav").read_bytes(), i


def test_single_stream_logits_against_oracle(device, files):
    """Teacher-forced logits of T's single-stream decode against the oracle over 150 positions,
    with test_lfm2_gpu.py's bounds: per-position max-rel <= 5e-2, argmax agreement >= 95 %. No
    exactness at early positions (test_llm_gpu.py lets BF16 flip from position 0)."""
    g = m.Llm(device, files["T"], 256)
    o = pyoracle.Llm(files["T"], 256)
    toks = np.random.default_rng(7).integers(0, g.n_vocab, 150)
    agree, rels = 0, []
    for pos, t in enumerate(toks):
        lg, lo = g.eval(int(t), pos), o.eval(int(t), pos)
        rels.append(float(np.abs(lg - lo).max() / np.abs(lo).max()))
        agree += int(lg.argmax() == lo.argmax())
    g.close()
    print(f"T single-stream: max rel {max(rels):.3g} (pos {int(np.argmax(rels))}), median {np.median(rels):.3g}, "
          f"argmax agree {agree}/150")
    assert max(rels) <= 5e-2, (int(np.argmax(rels)), max(rels))
    assert agree >= 0.95 * 150, agree
