"""CPU: the sampler chain's C-ABI without a GPU: NULL handles are refused with MIO_ERR_INVALID and
a message, the struct the binding passes has the header's layout, and the CLI refuses bad values
before it loads anything."""
import ctypes
import os
import subprocess

import miotts_amd as m

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "miotts-llama.cpp_amd", "build")


def test_null_handle_is_refused():
    L = m.lib()
    s = m.Sampling(top_k=40)
    assert L.mio_hip_llm_set_sampling(None, ctypes.byref(s)) == -1
    assert b"null" in L.mio_hip_last_error()
    assert L.mio_hip_llm_set_sampling(None, None) == -1
    assert L.mio_hip_llm_get_sampling(None, ctypes.byref(s)) == -1
    tok = ctypes.c_int32(0)
    row = (ctypes.c_float * 4)()
    assert L.mio_hip_llm_debug_sample_chain(None, row, None, 0, ctypes.byref(s), 0.8, 42, 0, 0, 4, ctypes.byref(tok),
                                            None, None, None) == -1


def test_sampling_struct_layout_and_defaults():
    assert ctypes.sizeof(m.Sampling) == 28
    assert [f for f, _ in m.Sampling._fields_] == ["top_k", "top_p", "min_p", "repeat_penalty", "frequency_penalty",
                                                   "presence_penalty", "repeat_last_n"]
    assert m.Sampling().as_dict() == dict(top_k=0, top_p=1.0, min_p=0.0, repeat_penalty=1.0, frequency_penalty=0.0,
                                          presence_penalty=0.0, repeat_last_n=64)
    src = open(os.path.join(m.INCLUDE_DIR, "mio_hip.h"), encoding="utf-8").read()
    assert "typedef struct mio_sampling" in src and "mio_hip_llm_set_sampling" in src


def test_cli_refuses_bad_sampling_values():
    base = [os.path.join(BIN, "miotts"), "-m", "x.gguf", "-c", "y.gguf", "-v", "z.gguf", "-p", "x"]
    for flags, text in ((["--top-k", "many"], "Invalid value for --top-k"), (["--top-p", "0.9x"], "Invalid value"),
                        (["--repeat-penalty", "0"], "--repeat-penalty must be > 0"),
                        (["--repeat-last-n", "300"], "--repeat-last-n must be in 0..256")):
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and text in p.stderr, (flags, p.returncode, p.stderr[-500:])
    p = subprocess.run([os.path.join(BIN, "miotts"), "--help"], capture_output=True, text=True, timeout=60)
    for flag in ("--top-k", "--top-p", "--min-p", "--repeat-penalty", "--repeat-last-n", "--frequency-penalty",
                 "--presence-penalty"):
        assert flag in p.stderr, flag
