#!/usr/bin/env python3
"""Which kernels compile differently between two trees?  Compares two directories of emitted ISA (the <unit>.s files that
`tools/asm_operand_overlap.py --keep DIR` leaves) kernel by kernel: instruction text with comments dropped and the
function index of local labels (.LBB<f>_<n>) normalised, so that adding a kernel to a unit does not "change" the others.
For every kernel whose instructions differ it prints both sides' instruction count, registers, scratch, LDS and occupancy
(the figures of the listing's "Kernel info" trailer, the same numbers tools/kernel_meta.py reads from the code object).

usage: python tools/isa_kernel_diff.py OLD_DIR NEW_DIR [--out FILE]"""
import argparse
import os
import re
import subprocess
import sys

_SYMBOL = re.compile(r"^([A-Za-z_$.][\w$.]*):\s*; @")
_INFO = {"vgpr": r"; NumVgprs: (\d+)", "agpr": r"; NumAgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)", "scratch": r"; ScratchSize: (\d+)",
         "lds": r"; LDSByteSize: (\d+)", "occupancy": r"; Occupancy: (\d+)"}


def kernels(path):
    """{symbol: (normalised instruction lines, {figure: value})} of one listing"""
    out, name, body = {}, None, []
    lines = open(path).read().splitlines()
    for i, line in enumerate(lines):
        m = _SYMBOL.match(line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            info, tail = {}, "\n".join(lines[i:i + 60])
            for k, pat in _INFO.items():
                mm = re.search(pat, tail)
                info[k] = int(mm.group(1)) if mm else -1
            out[name], name = (body, info), None
            continue
        s = line.split(";")[0].strip() if not line.strip().startswith(";;#") else ""
        if s and not s.startswith("."):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
        elif s.startswith(".LBB"):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old"); ap.add_argument("new"); ap.add_argument("--out")
    a = ap.parse_args()
    rows, same, added, removed = [], 0, [], []
    for unit in sorted(f for f in os.listdir(a.new) if f.endswith(".s")):
        new = kernels(os.path.join(a.new, unit))
        old = kernels(os.path.join(a.old, unit)) if os.path.exists(os.path.join(a.old, unit)) else {}
        for k, (body, info) in new.items():
            if k not in old:
                added.append((unit, k))
            elif old[k][0] == body:
                same += 1
            else:
                rows.append((unit, k, old[k], (body, info)))
        removed += [(unit, k) for k in old if k not in new]
    names = [k for _, k, _, _ in rows]
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines())) if names else {}
    fmt = lambda b, i: "%6d instr  vgpr %3d agpr %3d sgpr %3d scratch %4d lds %6d occupancy %d" % (len(b), i["vgpr"], i["agpr"], i["sgpr"], i["scratch"], i["lds"], i["occupancy"])
    text = ["%d kernels / device functions with identical instructions, %d changed, %d only in the new tree, %d only in the old" % (same, len(rows), len(added), len(removed))]
    for unit, k, (ob, oi), (nb, ni) in rows:
        text.append("%s  %s" % (unit[:-2], re.sub(r"^void ", "", dem.get(k, k)).split("(")[0]))
        text.append("    old " + fmt(ob, oi))
        text.append("    new " + fmt(nb, ni) + ("   <-- scratch or occupancy differs" if (oi["scratch"], oi["occupancy"]) != (ni["scratch"], ni["occupancy"]) else ""))
    for unit, k in removed:
        text.append("only in the old tree: %s %s" % (unit[:-2], k))
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
