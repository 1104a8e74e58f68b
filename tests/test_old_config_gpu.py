"""GPU: a program compiled against include/test-to-speech.h as it was before
Config::output_sample_rate (made here by cutting the field and Config's ABI tag out of the current
header; compiled unoptimised so the fill of Config's tail padding stays) binds to the untagged
constructor the library keeps and writes the codec's own rate, whatever those bytes hold."""
import os
import re
import subprocess

import numpy as np
import pytest

import miotts_amd as m

pytestmark = pytest.mark.gpu
BIN = os.path.join(m.PKG_ROOT, "build")


def test_caller_built_before_the_output_rate(tmp_path):
    src = open(os.path.join(m.INCLUDE_DIR, "test-to-speech.h"), encoding="utf-8").read()
    old, n = re.subn(r"[ \t]*// extension: the rate of everything written.*?int output_sample_rate = 0;\n", "", src,
                     flags=re.S)
    old, k = re.subn(r"\[\[gnu::__abi_tag__\(\"cfg2\"\)\]\] ", "", old)
    assert n == 1 and k == 1 and "output_sample_rate = " not in old and "int device = -1;" in old
    (tmp_path / "test-to-speech.h").write_text(old, "utf-8")
    exe, caller = str(tmp_path / "caller"), os.path.join(os.path.dirname(__file__), "old_config_caller.cpp")
    subprocess.run(["g++", "-O0", "-std=c++17", f"-I{tmp_path}", caller, "-o", exe, f"-L{BIN}", "-lmiotts",
                    f"-Wl,-rpath,{BIN}"], check=True, capture_output=True, text=True, timeout=120)
    codec, voice = m.synth_codec(str(tmp_path / "c.gguf"), 1, 1), m.synth_voice(str(tmp_path / "v.emb.gguf"), 7)
    text = "".join(f"<|s_{c}|>" for c in np.random.default_rng(3).integers(0, 12800, 30))
    runs = [[os.path.join(BIN, "miotts"), "-c", codec, "-v", voice, "--skip-llm", "-p", text, "-o", str(tmp_path / "cli.wav")]]
    runs += [[exe, codec, voice, text, str(tmp_path / f"old_{fill}.wav"), str(fill)] for fill in (0, 255)]
    for cmd in runs:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (cmd[0], p.stderr[-1500:])
    for fill in (0, 255):
        assert (tmp_path / f"old_{fill}.wav").read_bytes() == (tmp_path / "cli.wav").read_bytes(), fill
