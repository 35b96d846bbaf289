#!/usr/bin/env python3
"""Operand-overlap scan of the inline assembly, on the emitted gfx950 ISA (no GPU needed).

A multi-instruction `asm` statement whose read-write operands are not early-clobber ("+v" instead of "+&v") lets the
compiler give an INPUT the register of such an operand when it can prove both hold the same value (a literal zero word
and the zero-initialised carry word of the Montgomery product, say).  The statement's first write to that register then
changes the input before a later instruction of the same statement reads it.  Nothing in the source shows this; the ISA
does.  This tool emits the device ISA of the library's translation units (the Makefile's CXXFLAGS plus
`--cuda-device-only -S`) and, inside every `;;#ASMSTART ... ;;#ASMEND` block,

  * tracks the vector registers written as DESTINATIONS of multiply-adds (v_mad_u64_u32) and of add / subtract
    instructions with carry (v_add_co / v_addc_co / v_sub_co / v_subb_co and their rev forms);
  * reports every v_mad_u64_u32 one of whose two multiplicand registers was written earlier in the block and is neither
    the instruction's destination nor its accumulator;
  * in blocks without a multiply-add (the carry chains of add / sub), reports every add / subtract-with-carry source
    register written earlier in the block that is not the instruction's own destination.

It reads the register operands of those opcodes and nothing else.

usage: python tools/asm_operand_overlap.py [--src CSRC_DIR] [--units a.hip ...] [--jobs N] [--keep DIR] [--label TEXT] [--out FILE]
  --src    the csrc directory to compile (default: this tree's uzkge_amd/csrc); another checkout's to compare against
  --keep   keep the emitted <unit>.s files there (tools/isa_kernel_diff.py compares two such directories)
  --out    write the report into FILE as the section of its --label, replacing a section of the same label
           (profiles/asm_operand_overlap.txt holds the parent's, this tree's and the hooks' on the parent's assembly)
Exit status 1 when an overlapped read is found."""
import argparse
import collections
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uzkge_amd", "csrc")
MAX_JOBS = 16

MAD = "v_mad_u64_u32"
CARRY = ("v_add_co_u32", "v_addc_co_u32", "v_sub_co_u32", "v_subb_co_u32", "v_subrev_co_u32", "v_subbrev_co_u32")
_SYMBOL = re.compile(r"^([A-Za-z_$.][\w$.]*):\s*; @")
_VREG = re.compile(r"^v(\d+)$")
_VRANGE = re.compile(r"^v\[(\d+):(\d+)\]$")

Finding = collections.namedtuple("Finding", "kernel line_no text registers")


def vregs(operand):
    """The vector registers an operand names: v7 -> {7}, v[4:5] -> {4, 5}, anything else (vcc, s3, 0, -1) -> {}."""
    operand = operand.strip()
    m = _VREG.match(operand)
    if m:
        return {int(m.group(1))}
    m = _VRANGE.match(operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def _carry_opcode(op):
    return any(op == c or op.startswith(c + "_") for c in CARRY)


def scan_block(kernel, lines):
    """lines: [(line_no, text)] of one asm block.  -> [Finding]"""
    ins = []
    for no, text in lines:
        body = text.split(";")[0].strip()
        if not body:
            continue
        parts = body.split(None, 1)
        op = parts[0]
        if op == MAD or op.startswith(MAD + "_") or _carry_opcode(op):
            ins.append((no, body, op, [o.strip() for o in (parts[1] if len(parts) > 1 else "").split(",")]))
    has_mad = any(op.startswith(MAD) for _, _, op, _ in ins)
    written, found = set(), []
    for no, body, op, ops in ins:
        dst = vregs(ops[0]) if ops else set()
        if op.startswith(MAD):
            # v_mad_u64_u32 dst, carry_out, src0, src1, accumulator
            if len(ops) >= 5:
                bad = ((vregs(ops[2]) | vregs(ops[3])) & written) - dst - vregs(ops[4])
                if bad:
                    found.append(Finding(kernel, no, body, tuple(sorted(bad))))
        elif not has_mad:
            # v_addc_co_u32 dst, carry_out, src0, src1[, carry_in]
            srcs = set()
            for o in ops[2:4]:
                srcs |= vregs(o)
            bad = (srcs & written) - dst
            if bad:
                found.append(Finding(kernel, no, body, tuple(sorted(bad))))
        written |= dst
    return found


def scan_text(text):
    """ISA listing -> ([Finding], number of symbols seen, number of asm blocks seen)."""
    kernel, block, found, symbols, blocks = "?", None, [], 0, 0
    for no, line in enumerate(text.splitlines(), 1):
        m = _SYMBOL.match(line)
        if m:
            kernel, symbols = m.group(1), symbols + 1
            continue
        s = line.strip()
        if s.startswith(";;#ASMSTART"):
            block = []
        elif s.startswith(";;#ASMEND"):
            if block is not None:
                blocks += 1
                found += scan_block(kernel, block)
            block = None
        elif block is not None:
            block.append((no, s))
    return found, symbols, blocks


def makefile_flags(csrc):
    """CXXFLAGS of the library's Makefile with $(ARCH) filled in, and the sources behind its OBJS."""
    text = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1).strip()
    flags = shlex.split(var("CXXFLAGS").replace("$(ARCH)", var("ARCH")))
    units = []
    for obj in var("OBJS").split():
        stem = obj[:-2]
        units.append(stem + (".hip" if os.path.exists(os.path.join(csrc, stem + ".hip")) else ".cpp"))
    return var("HIPCC"), flags, units


def emit_isa(csrc, unit, outdir, hipcc, flags):
    out = os.path.join(outdir, os.path.splitext(unit)[0] + ".s")
    cmd = [hipcc] + flags + ["-w", "-DUZK_SRC_HASH=\"scan\"", "--cuda-device-only", "-S", "-x", "hip", unit, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s failed:\n%s" % (" ".join(cmd), r.stderr[-2000:]))
    return out


def scan_units(csrc=CSRC, units=None, jobs=MAX_JOBS, keep=None):
    """-> {unit: ([Finding], symbols, blocks)}"""
    hipcc, flags, all_units = makefile_flags(csrc)
    units = list(units) if units else all_units
    jobs = max(1, min(int(jobs), MAX_JOBS, len(units)))
    tmp = None if keep else tempfile.TemporaryDirectory()
    try:
        outdir = keep or tmp.name
        os.makedirs(outdir, exist_ok=True)
        with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
            paths = list(pool.map(lambda u: emit_isa(csrc, u, outdir, hipcc, flags), units))
        return {u: scan_text(open(p).read()) for u, p in zip(units, paths)}
    finally:
        if tmp is not None:
            tmp.cleanup()


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def report(results, label):
    lines = ["== %s" % label]
    total = 0
    for unit, (found, symbols, blocks) in results.items():
        per = collections.OrderedDict()
        for f in found:
            per.setdefault(f.kernel, []).append(f)
        total += len(found)
        lines.append("%-14s %4d functions, %5d asm blocks, %d kernels with overlapped reads" % (unit, symbols, blocks, len(per)))
        names = demangle(list(per))
        for k, fs in per.items():
            short = re.sub(r"^void ", "", names.get(k, k)).split("(")[0]
            lines.append("    %-70s %4d reads; first (line %d): %s" % (short, len(fs), fs[0].line_no, fs[0].text))
    lines.append("total: %d overlapped reads" % total)
    return "\n".join(lines) + "\n", total


def write_section(path, text):
    """Put the report into `path` as the section of its label ("== label" up to the next "== "): a section of the same label is
    replaced where it stands, a new one goes to the end, so neither a second run nor the order of the runs changes the file."""
    label = text.splitlines()[0]
    old = open(path).read() if os.path.exists(path) else ""
    parts = re.split(r"(?m)^(?=== )", old)
    for i, part in enumerate(parts):
        if part.splitlines()[:1] == [label]:
            parts[i] = text + ("\n" if i + 1 < len(parts) else "")
            break
    else:
        if old and not old.endswith("\n\n"):
            parts.append("\n" if old.endswith("\n") else "\n\n")
        parts.append(text)
    with open(path, "w") as f:
        f.write("".join(parts))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--src", default=CSRC)
    ap.add_argument("--units", nargs="*")
    ap.add_argument("--jobs", type=int, default=MAX_JOBS)
    ap.add_argument("--keep")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--out")
    a = ap.parse_args()
    text, total = report(scan_units(a.src, a.units, a.jobs, a.keep), a.label)
    sys.stdout.write(text)
    if a.out:
        write_section(a.out, text)
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
