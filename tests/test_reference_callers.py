"""The drop-in boundary as a tested fact: the reference's OWN command-line programs
(/root/reference/src/main.cpp, examples/stream-benchmark.cpp, examples/stream-compare.cpp),
compiled unchanged against this repo's include/ and linked to libmiotts.so in place of
llama.cpp/ggml + src/*.cpp (`make -C oracle callers`, output only
in oracle/_ref/callers/, git-ignored). examples/stream-to-device.cpp needs miniaudio, which
the snapshot lacks, so it is not built.

CPU part (this file): the three programs build and link; every option the reference's usage
text lists is accepted by the repo's own CLIs (csrc/tools/*) under the same name; usage
errors and --help give the same exit codes and the same first error line; without a GPU
both fail the same way (exit 1, the same messages: there is no CPU fallback). What the
reference's programs did is recorded in tests/golden/reference_cli.json (option names, exit
codes, messages), so the repo's CLIs are held to it on every machine; where the reference's
sources are present the programs are also built and run, and must behave as recorded. The GPU part,
tests/test_reference_callers_gpu.py, runs the reference's programs on synthetic models and
compares their output files byte for byte with the repo's CLIs.
"""
import json
import os
import subprocess
import sys

import pytest

import miotts_amd as m

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "miotts-llama.cpp_amd", "build")
CALLERS = os.path.join(REPO, "oracle", "_ref", "callers")
GOLDEN = os.path.join(REPO, "tests", "golden")
PAIRS = [("miotts", "main.cpp"), ("miotts-stream-benchmark", "stream-benchmark.cpp"),
         ("miotts-stream-compare", "stream-compare.cpp")]


def _golden():
    sys.path.insert(0, GOLDEN)
    import make_golden
    return make_golden


@pytest.fixture(scope="module")
def recorded():
    """name -> what the reference's program did (tests/golden/reference_cli.json, written by
    `make_golden.py reference_cli` from the programs built here)."""
    with open(os.path.join(GOLDEN, "reference_cli.json"), encoding="utf-8") as f:
        rec = json.load(f)
    assert sorted(rec) == sorted(n for n, _ in PAIRS)
    return rec


@pytest.fixture(scope="module")
def callers():
    """oracle/_ref/callers/ where the reference's programs are built (built now if its sources are
    here), else None: the tests then stand on the record alone."""
    if os.path.isdir("/root/reference/src"):
        subprocess.check_call(["make", "-s", "-C", os.path.join(REPO, "oracle"), "callers"])
    if not all(os.path.exists(os.path.join(CALLERS, n)) for n, _ in PAIRS):
        return None
    return CALLERS


def _run(path, args):
    p = subprocess.run([path] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("name,src", PAIRS)
def test_reference_cli_options_are_accepted(callers, recorded, name, src):
    g, rec = _golden(), recorded[name]
    if callers:  # the live build of the reference's program behaves as recorded
        rc_ref, out_ref, err_ref = _run(os.path.join(callers, name), ["--help"])
        assert rc_ref == rec["help_rc"] and sorted(g.cli_flags(out_ref + err_ref)) == rec["flags"]
    rc_ours, out_ours, err_ours = _run(os.path.join(BIN, name), ["--help"])
    assert rec["help_rc"] == rc_ours == 0
    ref_flags = set(rec["flags"])
    assert {"-m", "--model", "-c", "--codec", "-v", "--voice", "-p", "--prompt", "-h", "--help"} <= ref_flags
    missing = ref_flags - g.cli_flags(out_ours + err_ours)
    assert not missing, f"{src} options the repo's {name} does not list: {sorted(missing)}"


@pytest.mark.parametrize("name,src", PAIRS)
@pytest.mark.parametrize("args", [[], ["--bogus"], ["-c", "x.gguf"], ["-p", "hi"], ["--max-tokens"]])
def test_reference_cli_usage_errors_match(callers, recorded, name, src, args):
    g = _golden()
    rec = [r for r in recorded[name]["usage_errors"] if r["args"] == args]
    assert len(rec) == 1, args
    rc_ref, out_ref, first_ref = rec[0]["rc"], rec[0]["stdout"], rec[0]["first_err"]
    if callers:
        rc_live, out_live, err_live = _run(os.path.join(callers, name), args)
        assert (rc_live, out_live, g.cli_first_err(err_live)) == (rc_ref, out_ref, first_ref)
    rc_ours, out_ours, err_ours = _run(os.path.join(BIN, name), args)
    assert rc_ref == rc_ours != 0, (rc_ref, rc_ours)
    assert out_ref == out_ours
    if first_ref != "Usage:":
        assert first_ref == g.cli_first_err(err_ours)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("refcallers")
    return {"llm": m.synth_llm(str(d / "llm.gguf"), 0, 1), "codec": m.synth_codec(str(d / "codec.gguf"), 1, 1),
            "voice": m.synth_voice(str(d / "voice.emb.gguf"), 7), "dir": d}


def _no_gpu():
    try:
        return m.device_count() == 0
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-GPU failure path")
@pytest.mark.parametrize("name,extra", [("miotts", ["-o", "x.wav"]), ("miotts-stream-benchmark", []),
                                        ("miotts-stream-compare", [])])
def test_reference_cli_without_gpu_fails_loudly(callers, recorded, models, name, extra):
    args = ["-m", models["llm"], "-c", models["codec"], "-v", models["voice"], "-p", "hello",
            "--max-tokens", 8] + extra
    rec = recorded[name]["no_gpu"]
    rc_ref, out_ref, err_ref = rec["rc"], rec["stdout"], rec["stderr"]
    if callers:
        assert _run(os.path.join(callers, name), args) == (rc_ref, out_ref, err_ref)
    rc_ours, out_ours, err_ours = _run(os.path.join(BIN, name), args)
    assert rc_ref == rc_ours == 1
    assert out_ref == out_ours and err_ref == err_ours
    assert "no HIP device" in err_ref


def test_miotts_batch_flags(tmp_path):
    """The batch extension of `miotts` (--batch FILE, --gpus N): listed in
    --help, --gpus without --batch and an unreadable or empty --batch file are usage errors
    (exit 1 with a message) before any device is touched."""
    exe = os.path.join(BIN, "miotts")
    rc, out, err = _run(exe, ["--help"])
    assert rc == 0 and "--batch" in out + err and "--gpus" in out + err
    common = ["-c", "c.gguf", "-v", "v.gguf", "-m", "m.gguf"]
    rc, _, err = _run(exe, common + ["-p", "x", "--gpus", "2"])
    assert rc == 1 and "--gpus needs --batch" in err
    rc, _, err = _run(exe, common + ["--batch", str(tmp_path / "missing.txt")])
    assert rc == 1 and "cannot read --batch file" in err
    (tmp_path / "empty.txt").write_text("\n\n")
    rc, _, err = _run(exe, common + ["--batch", str(tmp_path / "empty.txt")])
    assert rc == 1 and "has no prompts" in err
