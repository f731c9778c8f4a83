#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?  For a change that moves code between translation units and must not change what any kernel compiles to.

usage: tools/compare_kernels.py --old OLD.o [OLD2.o ...] --new NEW.o [NEW2.o ...]

Each argument is what `hipcc <the product flags of _build.py> --cuda-device-only -c unit.hip` writes (an offload bundle, unbundled here with clang-offload-bundler) or
a gfx950 code object.  A kernel is a function symbol with a descriptor (<name>.kd).  Every kernel of the old set must be in exactly one object of the new set, and
no other (functions that are no kernels — device functions that were not inlined — are compared by name in every object that has them); for each the script compares
  * the bytes of its function, its pc-relative addresses (calls of device functions that were not inlined, tables) taken by the name of what they point at,
  * its resource symbols (<name>.num_vgpr, .num_agpr, .numbered_sgpr, .private_seg_size, .uses_vcc, ...),
  * its 64-byte descriptor, but for the one field that is a distance inside the object: the entry point's offset from the descriptor (bytes 16..23), which is
    checked to point at the function in both.
Where the bytes differ it prints a diff of the two disassemblies (llvm-objdump, addresses removed).  Exit status 1 if anything differs."""
import argparse
import difflib
import os
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hip-amdgcn-amd-amdhsa--gfx950"


def code_object(path, tmp):
    """the path of the ELF code object in `path` (itself, or unbundled into tmp)"""
    with open(path, "rb") as f:
        magic = f.read(24)
    if magic.startswith(b"\x7fELF"):
        return path
    assert magic.startswith(b"__CLANG_OFFLOAD_BUNDLE__"), "%s: neither a code object nor an offload bundle" % path
    out = os.path.join(tmp, "%d_%s.co" % (len(os.listdir(tmp)), os.path.basename(path)))
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + path, "--output=" + out], check=True)
    return out


class Elf:
    def __init__(self, path):
        self.path = path
        self.data = d = open(path, "rb").read()
        assert d[:6] == b"\x7fELF\x02\x01", path  # 64-bit, little endian
        shoff, = struct.unpack_from("<Q", d, 0x28)
        shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
        self.sections = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]  # name, type, flags, addr, offset, size, link, info, align, entsize
        self.symbols = {}
        for sec in self.sections:
            if sec[1] != 2:  # SHT_SYMTAB
                continue
            stroff = self.sections[sec[6]][4]
            for off in range(sec[4], sec[4] + sec[5], 24):
                name, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", d, off)
                end = d.index(b"\0", stroff + name)
                self.symbols[d[stroff + name:end].decode()] = (value, size, shndx, info & 15)

    def bytes_of(self, name):
        value, size, shndx, _ = self.symbols[name]
        sec = self.sections[shndx]
        return self.data[sec[4] + value - sec[3]:sec[4] + value - sec[3] + size]

    def symbol_at(self, addr):
        for n, (value, size, shndx, typ) in self.symbols.items():
            if typ in (1, 2) and shndx not in (0, 0xFFF1) and value <= addr < value + max(size, 1):  # an object or a function
                return "%s+%d" % (n, addr - value)
        return None  # (reported as a difference)

    def code_of(self, name):
        """The function's bytes with every pc-relative address taken out, and those addresses by name.  The compiler reaches another function or a table through
        s_getpc_b64 sN / s_add_u32 sN, sN, lo / s_addc_u32 sN+1, sN+1, hi: lo and hi are the target's distance from the s_add_u32, which changes whenever the object's
        layout does.  The two literals are zeroed in the copy and the target is returned as 'symbol+offset'."""
        code = bytearray(self.bytes_of(name))
        base = self.symbols[name][0]
        dw = struct.unpack_from("<%dI" % (len(code) // 4), code)
        refs = []
        for i in range(len(dw) - 4):
            if dw[i] & 0xFF80FF00 == 0xBE801C00 and dw[i + 1] & 0xFF80FF00 == 0x8000FF00 and dw[i + 3] & 0xFF80FF00 == 0x8200FF00:
                dist = dw[i + 2] | dw[i + 4] << 32
                dist -= (dist >> 63) << 64
                refs.append((4 * i, self.symbol_at(base + 4 * i + 4 + dist)))
                code[4 * i + 8:4 * i + 12] = code[4 * i + 16:4 * i + 20] = bytes(4)
        return bytes(code), refs

    def kernels(self):
        return sorted(n for n, s in self.symbols.items() if s[3] == 2 and n + ".kd" in self.symbols)  # STT_FUNC with a descriptor

    def other_functions(self):
        return sorted(n for n, s in self.symbols.items() if s[3] == 2 and s[2] != 0 and n + ".kd" not in self.symbols)

    def resources(self, kernel):
        return {n[len(kernel):]: s[0] for n, s in self.symbols.items() if n.startswith(kernel + ".") and s[2] == 0xFFF1}  # SHN_ABS

    def descriptor(self, kernel):
        kd = bytearray(self.bytes_of(kernel + ".kd"))
        assert len(kd) == 64, (kernel, len(kd))
        entry, = struct.unpack_from("<q", kd, 16)
        points_at_function = self.symbols[kernel + ".kd"][0] + entry == self.symbols[kernel][0]
        kd[16:24] = bytes(8)
        return bytes(kd), points_at_function

    def disassembly(self, name):
        value, size, _, _ = self.symbols[name]
        out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", "--start-address=%d" % value, "--stop-address=%d" % (value + size), self.path],
                             stdout=subprocess.PIPE, text=True, check=True).stdout
        return [l.split("//")[0].rstrip() for l in out.splitlines() if l.startswith("\t")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="compare_kernels_")
    try:
        old = [Elf(code_object(p, tmp)) for p in a.old]
        new = [Elf(code_object(p, tmp)) for p in a.new]
        bad = 0
        where = {}
        for side, elfs, paths in (("old", old, a.old), ("new", new, a.new)):
            for e, p in zip(elfs, paths):
                ks = e.kernels()
                print("%s %s: %d kernels, %d other functions%s" % (side, p, len(ks), len(e.other_functions()), "".join("\n    " + f for f in e.other_functions())))
                for k in ks:
                    where.setdefault((side, k), []).append(e)
        for (side, k), es in sorted(where.items()):
            if len(es) != 1:
                bad += 1
                print("DEFINED %d TIMES in the %s set: %s" % (len(es), side, k))
        names_old, names_new = {k for s, k in where if s == "old"}, {k for s, k in where if s == "new"}
        for k in sorted(names_old - names_new):
            bad += 1
            print("LOST: %s" % k)
        for k in sorted(names_new - names_old):
            bad += 1
            print("ADDED: %s" % k)
        compared = differ = 0
        for k in sorted(names_old & names_new):
            o, n = where[("old", k)][0], where[("new", k)][0]
            compared += 1
            what = []
            (co, ro), (cn, rn) = o.code_of(k), n.code_of(k)
            if co != cn:
                what.append("code (%d and %d bytes)" % (len(co), len(cn)))
            elif ro != rn or None in [t for _, t in ro + rn]:
                what.append("pc-relative targets %s" % [(a, b) for a, b in zip(ro, rn) if a != b][:4])
            if o.resources(k) != n.resources(k):
                what.append("resources %s -> %s" % (sorted(o.resources(k).items()), sorted(n.resources(k).items())))
            (kdo, oko), (kdn, okn) = o.descriptor(k), n.descriptor(k)
            if kdo != kdn or not oko or not okn:
                what.append("descriptor (entry points at the function: %s, %s)" % (oko, okn))
            if what:
                differ += 1
                print("DIFFERS: %s: %s" % (k, "; ".join(what)))
                if co != cn:
                    sys.stdout.writelines(l + "\n" for l in list(difflib.unified_diff(o.disassembly(k), n.disassembly(k), "old", "new", lineterm="", n=2))[:80])
        print("kernels: %d old, %d new, %d compared, %d differ" % (len(names_old), len(names_new), compared, differ))
        for e in new:  # the device functions that stayed functions: each copy against the old set's
            for f in e.other_functions():
                olds = [o for o in old if f in o.symbols]
                if not olds or any(o.code_of(f) != e.code_of(f) for o in olds):
                    differ += 1
                    print("DIFFERS: function %s of %s (%s)" % (f, e.path, "not in the old set" if not olds else "code"))
        return 1 if bad or differ else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
