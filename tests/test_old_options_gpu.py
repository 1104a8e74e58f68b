"""GPU: a program compiled against an earlier include/test-to-speech.h, whose TestToSpeech::Options
ends before the sampler chain's fields and has no ABI tag, still runs on this library: it binds to
the untagged entry points the library keeps (csrc/host/tts.cpp, "earlier entry points"), which
read the 12 bytes they are given and no more, so whatever follows the caller's object (zeros, ones)
is not taken for settings and the WAV has the bytes the CLI writes.

The earlier header is made here from the current one by cutting the tag and the chain's fields out
of Options; tests/old_options_caller.cpp is compiled against it and linked to build/libmiotts.so.
"""
import os
import re
import shutil
import subprocess

import pytest

import miotts_amd as m

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "miotts-llama.cpp_amd", "build")
HERE = os.path.dirname(os.path.abspath(__file__))


def test_caller_built_against_the_earlier_header(tmp_path):
    inc = tmp_path / "include"
    inc.mkdir()
    src = open(os.path.join(m.INCLUDE_DIR, "test-to-speech.h"), encoding="utf-8").read()
    old, n = re.subn(r"[ \t]*// extensions: the on-device sampler chain.*?float presence_penalty = 0.0f;\n", "", src,
                     flags=re.S)
    old, k = re.subn(r"\[\[gnu::abi_tag\(\"opt2\"\)\]\] ", "", old)
    assert n == 1 and k == 1 and "top_k" not in old and "abi_tag(" not in old and "ignore_eos" in old
    (inc / "test-to-speech.h").write_text(old, "utf-8")
    exe = tmp_path / "old_options_caller"
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    subprocess.run([cxx, "-O2", "-std=c++17", f"-I{inc}", os.path.join(HERE, "old_options_caller.cpp"), "-o", str(exe),
                    f"-L{BIN}", "-lmiotts", f"-Wl,-rpath,{BIN}"], check=True, capture_output=True, text=True, timeout=120)
    llm, codec = m.synth_llm(str(tmp_path / "llm1.gguf"), 1, 1), m.synth_codec(str(tmp_path / "codec.gguf"), 1, 1)
    voice = m.synth_voice(str(tmp_path / "voice.emb.gguf"), 7)
    p = subprocess.run([os.path.join(BIN, "miotts"), "-m", llm, "-c", codec, "-v", voice, "-p", "テストです。", "-o",
                        str(tmp_path / "cli.wav"), "--max-tokens", "40", "--speech-only", "--ignore-eos"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-1500:]
    want = (tmp_path / "cli.wav").read_bytes()
    for fill in (0, 255):
        out = tmp_path / f"old_{fill}.wav"
        p = subprocess.run([str(exe), llm, codec, voice, "テストです。", str(out), str(fill)], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, (fill, p.stderr[-1500:])
        assert out.read_bytes() == want, fill
