#!/usr/bin/env python3
"""Instruction counts along ONE executed path through a kernel's time-step loop in a gfx950 assembly file.
usage: tools/asm_path.py <file.s> <mangled kernel name> [label to take ...]
The loop is found as tools/asm_census.py finds it.  The walk starts at the loop head and ends at the backward branch:
s_branch is followed (also to blocks placed behind the loop), s_cbranch_execnz is taken and s_cbranch_execz is not (the
march kernels run with every lane active), every other conditional branch falls through unless its target is named on the
command line.  Use it where a loop holds both sides of a uniform branch and the static totals count both."""
import re
import sys

s = open(sys.argv[1]).read()
name, take = sys.argv[2], set(sys.argv[3:])
i = s.index("\n" + name + ":")
j = s.index(".Lfunc_end", i)
lines = [l.split(";")[0].strip() for l in s[i:j].split("\n")]
labels = {l[:-1]: k for k, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", l)}
best = None
for k, l in enumerate(lines):
    m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < k:
        if best is None or k - labels[m.group(1)] > best[1] - best[0]:
            best = (labels[m.group(1)], k)
head = best[0]
cnt = {"VALU": 0, "transcendental": 0, "16x16x32 MFMA": 0, "other MFMA": 0, "LDS": 0, "SALU": 0, "VMEM": 0}
seen_choices = []
k, steps = head + 1, 0
while steps < 100000:
    steps += 1
    l = lines[k]
    k += 1
    if not l or l.startswith(".") or l.endswith(":"):
        continue
    op = l.split()[0]
    m = re.match(r"(s_branch|s_cbranch_\w+)\s+(\.LBB\d+_\d+)", l)
    if m:
        cnt["SALU"] += 1
        kind, tgt = m.groups()
        go = kind == "s_branch" or kind == "s_cbranch_execnz" or (kind != "s_cbranch_execz" and tgt in take)
        if kind not in ("s_branch", "s_cbranch_execnz", "s_cbranch_execz"):
            seen_choices.append("%s %s: %s" % (kind, tgt, "taken" if go else "not taken"))
        if go:
            if labels[tgt] == head:
                break
            k = labels[tgt] + 1
        continue
    if op.startswith("v_mfma_f32_16x16x32"):
        cnt["16x16x32 MFMA"] += 1
    elif op.startswith("v_mfma"):
        cnt["other MFMA"] += 1
    elif op.startswith(("v_exp", "v_rcp", "v_log", "v_sqrt", "v_rsq")):
        cnt["transcendental"] += 1
    elif op.startswith("v_"):
        cnt["VALU"] += 1
    elif op.startswith("ds_"):
        cnt["LDS"] += 1
    elif op.startswith("s_"):
        cnt["SALU"] += 1
    else:
        cnt["VMEM"] += 1
print("path:", "; ".join(seen_choices))
print("  " + ", ".join("%s %d" % kv for kv in cnt.items()))
