#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libphnn_mpc.so, kernel by kernel (no GPU needed).

    python tools/isa_compare.py libA.so libB.so [--changed-only]

The gfx950 code objects are taken out of each library as tests/test_static_isa.py::_code_objects does (one per linked
translation unit, in the order of the Makefile's link rule) and disassembled with llvm-objdump; a file that is itself
a code object (one unit compiled with --cuda-device-only) is taken as it is.  Per unit and per
function symbol one line:
    IDENTICAL    the same instructions with the same operands in the same order
    ORDER ONLY   the same multiset of opcodes once s_nop / s_waitcnt are set aside (scheduling differs, work does not)
    DIFFERENT    anything else; the opcodes whose counts differ follow (count in A -> count in B)
A generic diff of two builds: it looks for no particular instruction.  --changed-only leaves the IDENTICAL lines out.
"""
import collections
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
PADDING = ("s_nop", "s_waitcnt")


def code_objects(path):
    blob = open(path, "rb").read()
    if blob[:4] == b"\x7fELF" and MAGIC not in blob:  # one unit built with --cuda-device-only: the code object itself
        return [blob]
    out, pos = [], blob.find(MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", blob, pos + len(MAGIC))[0]
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size > 0:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + len(MAGIC))
    return out


def linked_units():
    mk = open(os.path.join(ROOT, "phnn_mpc_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^libphnn_mpc\.so:(.*)$", mk, re.M)
    return [w[:-2] + ".hip" for w in rule.group(1).split() if w.endswith(".o")] if rule else []


def functions(image):
    """{demangled symbol: [instruction text without address and encoding]} of one code object, in file order."""
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "co.elf")
        open(f, "wb").write(image)
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", "--mcpu=gfx950", f],
                              capture_output=True, text=True, check=True).stdout
    funcs, cur = collections.OrderedDict(), None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    return funcs, hashlib.sha256(text.split("\n", 2)[-1].encode()).hexdigest()[:16]  # without the 'file format' line


def opcodes(insts):
    c = collections.Counter(i.split()[0] for i in insts if i)
    for k in PADDING:
        c.pop(k, None)
    return c


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    changed_only = "--changed-only" in sys.argv
    if len(args) != 2:
        sys.exit(__doc__)
    A, B = code_objects(args[0]), code_objects(args[1])
    units = linked_units()
    if len(A) != len(B):
        sys.exit(f"{len(A)} gfx950 code objects in {args[0]}, {len(B)} in {args[1]}: not builds of the same units")
    total = collections.Counter()
    for k, (a, b) in enumerate(zip(A, B)):
        unit = units[k] if len(units) == len(A) else f"unit {k}"
        fa, ha = functions(a)
        fb, hb = functions(b)
        tally, lines = collections.Counter(), []
        for name in list(fa) + [n for n in fb if n not in fa]:
            if name not in fa or name not in fb:
                cls, extra = "DIFFERENT", "  (only in %s)" % ("A" if name in fa else "B")
            elif fa[name] == fb[name]:
                cls, extra = "IDENTICAL", ""
            else:
                ca, cb = opcodes(fa[name]), opcodes(fb[name])
                if ca == cb:
                    cls, extra = "ORDER ONLY", ""
                else:
                    cls = "DIFFERENT"
                    extra = "  " + ", ".join(f"{op} {ca[op]}->{cb[op]}" for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op])
            tally[cls] += 1
            if cls != "IDENTICAL" or not changed_only:
                lines.append(f"  {cls:10s} {name}{extra}")
        total.update(tally)
        print(f"{unit}: code object {len(a)} / {len(b)} bytes{' (byte-identical)' if a == b else ''}, disassembly sha256 {ha} {hb}, "
              f"{len(fa)} / {len(fb)} functions: {tally['IDENTICAL']} IDENTICAL, {tally['ORDER ONLY']} ORDER ONLY, "
              f"{tally['DIFFERENT']} DIFFERENT")
        print("\n".join(lines)) if lines else None
    print(f"all units: {total['IDENTICAL']} IDENTICAL, {total['ORDER ONLY']} ORDER ONLY, {total['DIFFERENT']} DIFFERENT")
    return 0 if total["IDENTICAL"] == sum(total.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
