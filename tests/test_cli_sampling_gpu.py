"""GPU: the sampler chain's flags on the CLIs (csrc/tools/cli_args.h cli_common_flags ->
TestToSpeech::Options -> mio_hip_llm_set_sampling).

* `miotts --top-k 1 -t 0.8` keeps one id per step, so the noise has nothing to choose from: the WAV
  has the bytes `miotts -t 0` writes (greedy), through Options and the CLI, single and --batch.
* a value that is no number, or one the runner refuses, ends the tool with exit status 1 before
  any model is loaded; the streaming tools take the flags too.
"""
import os
import subprocess

import pytest

import miotts_amd as m

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "miotts-llama.cpp_amd", "build")


def run(args, timeout=300):
    p = subprocess.run([os.path.join(BIN, args[0])] + [str(a) for a in args[1:]], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, f"{args[0]} rc={p.returncode}\n{p.stdout}\n{p.stderr[-2000:]}"
    assert "batched decode unavailable" not in p.stderr, p.stderr[-2000:]
    return p.stdout


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_sampling")
    return {"llm": m.synth_llm(str(d / "llm1.gguf"), 1, 1), "codec": m.synth_codec(str(d / "codec_tiny.gguf"), 1, 1),
            "voice": m.synth_voice(str(d / "voice.emb.gguf"), 7), "dir": d}


def test_top_k_1_is_greedy(files):
    d = files["dir"]
    common = ["-m", files["llm"], "-c", files["codec"], "-v", files["voice"], "-p", "テストです。", "--max-tokens", 40,
              "--speech-only", "--ignore-eos"]
    run(["miotts"] + common + ["-t", 0, "-o", d / "greedy.wav"])
    run(["miotts"] + common + ["-t", 0.8, "--top-k", 1, "-o", d / "k1.wav"])
    run(["miotts"] + common + ["-t", 0.8, "-o", d / "t08.wav"])
    greedy = (d / "greedy.wav").read_bytes()
    assert (d / "k1.wav").read_bytes() == greedy
    assert (d / "t08.wav").read_bytes() != greedy, "T 0.8 without the chain equals greedy: the case shows nothing"
    # every flag at its neutral value: the bytes of a run without them
    run(["miotts"] + common + ["-t", 0.8, "--top-k", 0, "--top-p", 1, "--min-p", 0, "--repeat-penalty", 1,
                               "--repeat-last-n", 64, "--frequency-penalty", 0, "--presence-penalty", 0, "-o",
                               d / "neutral.wav"])
    assert (d / "neutral.wav").read_bytes() == (d / "t08.wav").read_bytes()
    # the batched path (synthesize_batch_to_files) takes the options too
    (d / "batch.txt").write_text("テストです。\nこんにちは。\n", "utf-8")
    run(["miotts"] + common + ["-t", 0.8, "--top-k", 1, "--batch", d / "batch.txt", "-o", d / "b.wav"])
    assert (d / "b_000.wav").read_bytes() == greedy


def test_bad_values_exit_1(files):
    base = [os.path.join(BIN, "miotts"), "-m", files["llm"], "-c", files["codec"], "-v", files["voice"], "-p", "x"]
    for flags, text in ((["--top-k", "many"], "Invalid value for --top-k"), (["--top-p", "0.9x"], "Invalid value"),
                        (["--repeat-penalty", "0"], "--repeat-penalty must be > 0"),
                        (["--repeat-last-n", "300"], "--repeat-last-n must be in 0..256"),
                        (["--min-p", "nan"], "NaN"), (["--presence-penalty"], "")):
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and text in p.stderr, (flags, p.returncode, p.stderr[-500:])


def test_stream_tools_take_the_flags(files):
    out = run(["miotts-stream-benchmark", "-m", files["llm"], "-c", files["codec"], "-v", files["voice"], "-p",
               "テストです。", "--max-tokens", 40, "--speech-only", "--ignore-eos", "--top-k", 40, "--top-p", 0.9,
               "--repeat-penalty", 1.1])
    assert "stream_bench.llm_tokens=40" in out, out[-1500:]
