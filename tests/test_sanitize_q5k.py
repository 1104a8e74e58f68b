"""Q5_K host code under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

tests/sanitize/q5k_host.cpp is a stand-alone program (its own main) linked with the product's
quant.cpp and gguf.cpp, built as test_sanitize_host.py builds its own: ROCm clang++,
-fsanitize=address,undefined -fno-sanitize-recover=all. It quantizes, dequantizes and re-packs
(split_layout / to_split) Q5_K rows at K in {256, 2304}, R in {1, 37} into buffers of exactly the
declared sizes, and must exit 0 with no report."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(REPO, "miotts-llama.cpp_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"  # g++ 11 has no _Float16 in C++ (quant.cpp)
SRCS = [os.path.join(REPO, "tests", "sanitize", "q5k_host.cpp"), os.path.join(H, "host", "quant.cpp"),
        os.path.join(H, "host", "gguf.cpp")]


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ (host build with sanitizers) absent")
def test_q5k_host_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "q5k_host")
    cmd = [CLANG, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(REPO, "include"), "-I" + H, "-I" + os.path.join(H, "host")] + SRCS + ["-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", OMP_NUM_THREADS="1"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    assert "q5k_host: clean" in p.stdout and not p.stderr.strip(), p.stderr[-2000:]
