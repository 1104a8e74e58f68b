"""CPU: the decode-step kernels' entry, read from the built gfx950 code objects.

The five launches of the flagship step (k_attn_in, k_att_o, k_layer_att, k_ffn, k_lm_head) begin
their parameter lists with an entry pack of plain pointers and ints (csrc/hip/llm_device.h,
"kernel entry") and are built with kernarg preload (the Makefile's KERNARG_PRELOAD). For the
1.7B Q4_K_M instantiation of each this checks, in the code object inside libmiotts.so:
  (i)   the kernel descriptor's kernarg preload length is the pack's dword count;
  (ii)  past the compiler's fallback prologue (the scalar loads of the pack for firmware that does
        not preload), on EVERY path from the kernel's entry that reaches a vector memory load, the
        first such load precedes the first `s_waitcnt lgkmcnt` (preload is kept): the x / norm
        weight / `done` loads of the matvec roles, and the StepState loads of the roles that take
        their work from the state (attention chunks and O workgroups from the position, layer 0's
        k_attn_in its x from `pending`), which are vector loads through the pack. On firmware
        that does not preload the prologue's one wait is the only scalar round in front of them.
        The same holds for the k_attn_in of the layers behind layer 0 (models whose attention
        block is not fused), checked beside the five. The parent: 1 to 3 waits before the first
        load, 1 to 6 before the first 16-byte load (profiles/entry_args/vgprs.txt);
  (iii) the kernarg segment is the parent's (db4e6ca, sizes below) plus the pack's bytes.
Skipped where the ROCm LLVM tools are absent.

    python tests/test_entry_args.py [libmiotts.so]
prints the figures (kernarg bytes, preload dwords, SGPRs, VGPRs, scratch, waits before the first
load) of a build, as kept in profiles/entry_args/vgprs.txt."""
import os
import re
import shutil
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "miotts-llama.cpp_amd", "build", "libmiotts.so")

# name -> (mangled-name fragment of the flagship instantiation, pack dwords, the parent's kernarg
# segment bytes); k_attn_in_rest: the instantiation of the layers behind layer 0
KERNELS = {
    "k_attn_in": ("9k_attn_inILi1ELi12ELi14ELi2ELb0ELb1EE", 8, 396),
    "k_attn_in_rest": ("9k_attn_inILi1ELi12ELi14ELi2ELb0ELb0EE", 8, 396),
    "k_att_o": ("7k_att_oILi128ELi2ELi1ELi12ELi1ELb0EE", 6, 272),
    "k_layer_att": ("11k_layer_attILi1ELi12ELi12ELi2ELi128ELi2ELi12ELi1ELb0EE", 10, 432),
    "k_ffn": ("5k_ffnILi1ELi12ELi6ELi3ELi14ELi3ELb0EE", 8, 600),
    "k_lm_head": ("9k_lm_headILi1ELi14ELb0EE", 8, 240),
}
PROLOGUE = 0x100  # the preload fallback prologue is padded to 256 bytes; the body starts behind it


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def code_objects(lib, workdir):
    """The gfx950 code objects embedded in `lib`, extracted into workdir."""
    objdump = _tool("llvm-objdump")
    copy = os.path.join(workdir, "lib.so")
    shutil.copy(lib, copy)
    subprocess.run([objdump, "--offloading", copy], check=True, capture_output=True, cwd=workdir)
    return sorted(os.path.join(workdir, f) for f in os.listdir(workdir) if "gfx950" in f)


def _sections(co):
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    text = subprocess.run([objdump, "-d", co], check=True, capture_output=True, text=True).stdout
    kd = subprocess.run([objdump, "-d", "-j", ".rodata", co], check=True, capture_output=True, text=True).stdout
    notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
    return text, kd, notes


def _body(text, frag):
    """[(offset, mnemonic, branch-target offset or None)] of the one function whose name holds frag."""
    m = [x for x in re.finditer(r"^([0-9a-f]+) <(\S+)>:\n", text, re.M) if frag in x.group(2) and "." not in x.group(2)]
    assert len(m) == 1, (frag, [x.group(2) for x in m])
    start, name = int(m[0].group(1), 16), m[0].group(2)
    end = text.find("\n\n", m[0].end())
    ins = []
    for line in text[m[0].end():end if end > 0 else len(text)].splitlines():
        r = re.match(r"\s+(\S+)(.*?)//\s*([0-9A-F]+):", line)
        if not r:
            continue
        t = re.search(r"<\S+?\+0x([0-9a-f]+)>\s*$", line)
        ins.append((int(r.group(3), 16) - start, r.group(1), int(t.group(1), 16) if t else None, r.group(2)))
    return name, ins


ANY_LOAD = ("buffer_load", "global_load")
WIDE_LOAD = ("buffer_load_dwordx4", "global_load_dwordx4")  # x, the norm weight, K / V rows, weights


def waits_before_first_load(ins, entry, loads=ANY_LOAD):
    """(fewest, most) `s_waitcnt lgkmcnt` a path from offset `entry` passes before its first
    vector load of the kinds `loads`, over every path that reaches one."""
    at = {off: i for i, (off, *_rest) in enumerate(ins)}
    best, worst, seen, todo = None, None, set(), [(at[entry], 0)]
    while todo:
        i, n = todo.pop()
        while i < len(ins) and (i, n) not in seen:
            seen.add((i, n))
            off, op, target, rest = ins[i]
            if op.startswith(loads):
                best = n if best is None else min(best, n)
                worst = n if worst is None else max(worst, n)
                break
            if op == "s_endpgm":
                break
            assert not op.startswith(("s_setpc", "s_swappc")), op
            if op == "s_waitcnt" and "lgkmcnt" in rest:
                n += 1
            if op == "s_branch":
                i = at[target]
                continue
            if op.startswith("s_cbranch"):
                todo.append((at[target], n))
            i += 1
    return best, worst


def kernel_facts(lib, workdir):
    """name -> dict(kernarg, preload, sgpr, vgpr, scratch, waits=(fewest, most)) of KERNELS in lib."""
    out = {}
    for co in code_objects(lib, workdir):
        text, kd, notes = _sections(co)
        for name, (frag, *_rest) in KERNELS.items():
            if frag not in text:
                continue
            sym, ins = _body(text, frag)
            d = kd[kd.index(".amdhsa_kernel " + sym):]
            d = d[:d.index(".end_amdhsa_kernel")]
            pre = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", d)
            # the metadata lists .private_segment_fixed_size, .sgpr_count ... .vgpr_count behind .name
            md = notes[re.search(r"\.name:\s+" + re.escape(sym) + r"\n", notes).end():][:600]
            f = {"kernarg": int(re.search(r"\.amdhsa_kernarg_size (\d+)", d).group(1)),
                 "preload": int(pre.group(1)) if pre else 0,
                 "scratch": int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d).group(1)),
                 "sgpr": int(re.search(r"\.sgpr_count:\s+(\d+)", md).group(1)),
                 "vgpr": int(re.search(r"\.vgpr_count:\s+(\d+)", md).group(1))}
            entry = PROLOGUE if f["preload"] else 0
            f["waits"] = waits_before_first_load(ins, entry)
            f["waits_wide"] = waits_before_first_load(ins, entry, WIDE_LOAD)
            out[name] = f
    return out


def _have_tools():
    return _tool("llvm-objdump") and _tool("llvm-readelf")


def _facts(tmp_path_factory):
    import pytest
    if not _have_tools():
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not found")
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built")
    f = kernel_facts(LIB, str(tmp_path_factory.mktemp("entry_args")))
    assert set(f) == set(KERNELS), sorted(set(KERNELS) - set(f))
    return f


try:
    import pytest

    @pytest.fixture(scope="module")
    def facts(tmp_path_factory):
        return _facts(tmp_path_factory)

    @pytest.mark.parametrize("name", sorted(KERNELS))
    def test_preload_length_is_the_pack(facts, name):
        assert facts[name]["preload"] == KERNELS[name][1], facts[name]

    @pytest.mark.parametrize("name", sorted(KERNELS))
    def test_first_load_precedes_the_first_scalar_wait(facts, name):
        fewest, most = facts[name]["waits"]
        print(name, facts[name])
        assert (fewest, most) == (0, 0), facts[name]

    @pytest.mark.parametrize("name", sorted(KERNELS))
    def test_kernarg_segment_grew_by_the_pack(facts, name):
        assert facts[name]["kernarg"] == KERNELS[name][2] + 4 * KERNELS[name][1], facts[name]

    @pytest.mark.parametrize("name", sorted(KERNELS))
    def test_no_scratch(facts, name):
        assert facts[name]["scratch"] == 0, facts[name]
except ImportError:  # the report below needs no pytest
    pass


if __name__ == "__main__":
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        for k, v in sorted(kernel_facts(sys.argv[1] if len(sys.argv) > 1 else LIB, d).items()):
            print(f"{k:12s} kernarg {v['kernarg']:4d} B  preload {v['preload']:2d} dwords  sgpr {v['sgpr']:3d}  "
                  f"vgpr {v['vgpr']:3d}  scratch {v['scratch']}  lgkmcnt waits before the first load: "
                  f"{v['waits'][0]} (best path) .. {v['waits'][1]} (worst), before the first 16-byte load: "
                  f"{v['waits_wide'][0]} .. {v['waits_wide'][1]}")
