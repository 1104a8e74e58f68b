"""Compare the device code of two builds of one .hip file, kernel by kernel.

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -c csrc/hip/X.hip -o X.co    (at each commit)
    python tools/kernel_bytes.py parent/X.co head/X.co

Each input is the gfx950 code object (an ELF, or the offload bundle that holds it). The whole
.text sections are compared first; when they differ (template instantiation order moves kernels
within the section), every function symbol's name, size and a hash of its bytes are. Nothing is
disassembled. Exit status 0: same kernels, same bytes."""
import hashlib
import struct
import sys

BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"


def code_object(path):
    data = open(path, "rb").read()
    if data.startswith(BUNDLE):
        n, = struct.unpack_from("<Q", data, 24)
        pos = 32
        for _ in range(n):
            off, size, tn = struct.unpack_from("<QQQ", data, pos)
            triple = data[pos + 24:pos + 24 + tn].decode()
            pos += 24 + tn
            if "gfx950" in triple:
                return data[off:off + size]
        raise SystemExit(f"{path}: no gfx950 entry in the bundle")
    assert data[:4] == b"\x7fELF", path
    return data


def sections(elf):
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    sh = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    strtab = sh[shstrndx]
    name = lambda o: elf[strtab[4] + o:elf.index(b"\0", strtab[4] + o)].decode()
    return [(name(s[0]),) + s for s in sh]


def functions(elf):
    """(.text bytes, {function symbol: (size, sha256 of its bytes)})"""
    secs = sections(elf)
    text = next(s for s in secs if s[0] == ".text")
    text_i = secs.index(text)
    symtab = next(s for s in secs if s[0] == ".symtab")
    strs = secs[symtab[7]]
    out = {}
    for i in range(symtab[6] // 24):
        st_name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, symtab[5] + i * 24)
        if info & 15 != 2 or shndx != text_i:  # STT_FUNC in .text
            continue
        nm = elf[strs[5] + st_name:elf.index(b"\0", strs[5] + st_name)].decode()
        off = text[5] + value - text[4]
        out[nm] = (size, hashlib.sha256(elf[off:off + size]).hexdigest())
    return elf[text[5]:text[5] + text[6]], out


def main(a, b):
    ta, fa = functions(code_object(a))
    tb, fb = functions(code_object(b))
    print(f"{a}: {len(fa)} functions, .text {len(ta)} bytes; {b}: {len(fb)} functions, .text {len(tb)} bytes")
    if ta == tb:
        print("identical .text sections")
        return 0
    bad = 0
    for nm in sorted(set(fa) | set(fb)):
        if nm not in fa or nm not in fb:
            print(("only in " + (a if nm in fa else b)) + ": " + nm)
        elif fa[nm] != fb[nm]:
            print(f"differs: {nm} size {fa[nm][0]} / {fb[nm][0]}")
        else:
            continue
        bad += 1
    print(".text sections differ; " + (f"{bad} function symbols differ" if bad else
                                       "every function symbol has the same name, size and bytes"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
