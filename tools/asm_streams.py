#!/usr/bin/env python3
"""What sits inside the 128 x 128 MFMA streams of one kernel's time-step loop in a gfx950 assembly file.
usage: tools/asm_streams.py <file.s> <mangled kernel name> [min MFMAs per stream = 90]
A stream is a run of v_mfma_f32_16x16x32 instructions with fewer than GAP other instructions between neighbours; for
every stream of at least the given length: its MFMA count and the VALU / transcendental / 4x4x1 MFMA / LDS instructions
between its first and last MFMA.  The loop is found as tools/asm_census.py finds it, and its totals are printed first."""
import re
import sys

GAP = 48
s = open(sys.argv[1]).read()
name = sys.argv[2]
min_len = int(sys.argv[3]) if len(sys.argv) > 3 else 90
i = s.index("\n" + name + ":")
j = s.index(".Lfunc_end", i)
lines = [l.split(";")[0].strip() for l in s[i:j].split("\n")]
labels = {l[:-1]: k for k, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", l)}
best = None
for k, l in enumerate(lines):
    m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.match(r"s_branch\s+(\.LBB\d+_\d+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < k:
        if best is None or k - labels[m.group(1)] > best[1] - best[0]:
            best = (labels[m.group(1)], k)
body = [l.split()[0] for l in lines[best[0]:best[1]] if l and not l.startswith((";", ".")) and not l.endswith(":")]


def kind(op):
    if op.startswith("v_mfma_f32_16x16x32"):
        return "M"
    if op.startswith("v_mfma"):
        return "m"
    if op.startswith(("v_exp", "v_rcp", "v_log", "v_sqrt", "v_rsq")):
        return "T"
    if op.startswith("v_"):
        return "V"
    if op.startswith("ds_"):
        return "L"
    return "o"


ks = [kind(op) for op in body]
print("loop: %d instructions, VALU %d, transcendental %d, 16x16x32 MFMA %d, other MFMA %d, LDS %d" % (
    len(ks), ks.count("V"), ks.count("T"), ks.count("M"), ks.count("m"), ks.count("L")))
pos = [k for k, c in enumerate(ks) if c == "M"]
streams, cur = [], []
for p in pos:
    if cur and p - cur[-1] > GAP:
        streams.append(cur)
        cur = []
    cur.append(p)
if cur:
    streams.append(cur)
tot_v = tot_t = 0
for st in streams:
    if len(st) < min_len:
        continue
    seg = ks[st[0]:st[-1] + 1]
    tot_v += seg.count("V")
    tot_t += seg.count("T")
    print("  stream at +%5d: %3d MFMAs, inside it VALU %3d, transcendental %3d, other MFMA %2d, LDS %3d" % (
        st[0], len(st), seg.count("V"), seg.count("T"), seg.count("m"), seg.count("L")))
print("  inside all streams: VALU %d, transcendental %d" % (tot_v, tot_t))
