#!/usr/bin/env python3
"""Inventory of the typed lazy 29-bit signatures the product instantiates (lz29.hpp's LzOps).

Every .hip translation unit under uzkge_amd/csrc that reaches lz29.hpp through its #include "..." lines -- directly or through any
chain of headers (g2msm.hip gets there by g2_29.hpp -> fq2_29.hpp) -- is parsed by clang (device side, -fsyntax-only) with its AST
dumped for LzOps; every used member instantiation of the operations below is one (field, operation, operand types, result type).
fieldops.hip is left out: it holds the test hooks, whose typed KAT ops and signature checks are not product code (and the latter
are generated from this very list).  The .cpp files stay in the source set: the Makefile compiles them as HIP (-x hip), so one that
reaches lz29.hpp (api.cpp, through g2_29.hpp for its wire structs) could instantiate LzOps the day it gains a kernel.  With the G2 group law (g2_29.hpp, fq2_29.hpp) the list
holds every typed operation of the G2 MSM's accumulator and XYZZ additions, the dual products with an un-normalised K = 4 operand
among them; with Anemoi-Jive (anemoi29.hpp, reached from anemoi.hip and from edwards.hip) the sums of its linear layer, up to
Lz<Fr29, 3, 837>.  The list is written as an X-macro next to lz29.hpp:

    LZ29_SIG(index, field, op, arity, Ka, Va, Kb, Vb, Kc, Vc, Kd, Vd, Kr, Vr)

unused operands are 0, 0; canon and to_wire return wire words (Kr = Vr = 0).  The test hook (fieldops.hip) instantiates the typed
sub / to_wire / canon of every entry, tests/lz29_contract.py parses the same file, and tests/test_lz29_contract.py regenerates it and
fails on any difference -- a new kernel cannot add a signature without a test of it.  Indices are stable: a signature already in
the committed file keeps its place and new ones are appended in sorted order (field, operation, types), so the G2-only entries
follow the 183 that the G1 and scalar kernels had before; written afresh, without a committed file, the list is simply sorted.

    python tools/lz29_inventory.py            # rewrite uzkge_amd/csrc/lz29_sigs.inc
    python tools/lz29_inventory.py --check    # exit 1 if the committed file differs
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uzkge_amd", "csrc")
OUT = os.path.join(CSRC, "lz29_sigs.inc")
OPS = ("add", "sub", "mul", "sqr", "mul2", "norm", "assume", "canon", "to_wire")
EXCLUDED = {"fieldops.hip"}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_FIELD = re.compile(r"TemplateArgument type 'uzk::Field29<uzk::(Fr|Fq)29Cfg>'")
_SPEC = re.compile(r"ClassTemplateSpecializationDecl .* struct LzOps definition")
_METHOD = re.compile(r"CXXMethodDecl .* used (\w+) '([^']*)' implicit_instantiation")
_TYPE = re.compile(r"E<([^<>]*)>")
_SIG = re.compile(r"^(Fp|E<[^<>]*>) \((.*)\)$")


_INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def reaches(path, target="lz29.hpp", seen=None):
    """Does the file include `target`, directly or through headers it includes (quoted includes, resolved next to the includer)?"""
    seen = set() if seen is None else seen
    path = os.path.normpath(path)
    if path in seen or not os.path.exists(path):
        return False
    seen.add(path)
    for inc in _INCLUDE.findall(open(path).read()):
        if os.path.basename(inc) == target or reaches(os.path.join(os.path.dirname(path), inc), target, seen):
            return True
    return False


def sources():
    return [name for name in sorted(os.listdir(CSRC))
            if name.endswith((".hip", ".cpp")) and name not in EXCLUDED and reaches(os.path.join(CSRC, name))]


def _int(expr: str) -> int:
    """A template argument as clang prints it (sums, prod_v(a, b), C integer division) -> its value."""
    py = expr.replace("/", "//")
    return int(eval(py, {"__builtins__": {}}, {"prod_v": lambda a, b: 1 + (a * b + 168) // 169}))


def _kv(arg: str):
    k, v = (s.strip() for s in _split_args(arg))
    return _int(k), _int(v)


def _split_args(s: str):
    depth, cur, parts = 0, "", []
    for ch in s:
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
            continue
        depth += ch == "("
        depth -= ch == ")"
        cur += ch
    parts.append(cur)
    return parts


def parse_ast(text: str):
    """(field, op, operand types, result type) of every used LzOps member instantiation in one AST dump."""
    sigs = set()
    field = None
    expect_field = False
    for line in text.splitlines():
        if _SPEC.search(line):
            expect_field, field = True, None
            continue
        m = _FIELD.search(line)
        if m and expect_field:
            field, expect_field = m.group(1).upper(), False
            continue
        m = _METHOD.search(line)
        if not m or field is None or m.group(1) not in OPS:
            continue
        op, sig = m.group(1), m.group(2)
        res, params = _SIG.match(sig).groups()
        args = tuple(_kv(t) for t in _TYPE.findall(params))
        r = (0, 0) if res == "Fp" else _kv(_TYPE.match(res).group(1))
        sigs.add((field, op, args, r))
    return sigs


def collect():
    sigs = set()
    for name in sources():
        cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "--cuda-device-only",
               "-x", "hip", "-fsyntax-only", "-Xclang", "-ast-dump", "-Xclang", "-ast-dump-filter", "-Xclang", "LzOps", os.path.join(CSRC, name)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"{name}: clang failed\n{res.stderr[-2000:]}")
        sigs |= parse_ast(res.stdout)
    return sorted(sigs, key=lambda s: (s[0], OPS.index(s[1]), s[2], s[3]))


_LINE = re.compile(r"^LZ29_SIG\((.*)\)\s*$", re.M)


def committed():
    """The signatures of the committed file, in its order (none if there is no file)."""
    out = []
    for body in _LINE.findall(open(OUT).read() if os.path.exists(OUT) else ""):
        f = [t.strip() for t in body.split(",")]
        arity, nums = int(f[3]), [int(t) for t in f[4:]]
        pairs = [(nums[2 * i], nums[2 * i + 1]) for i in range(5)]
        out.append((f[1], f[2], tuple(pairs[:arity]), pairs[4]))
    return out


def keep_indices(sigs, old):
    """An entry's index is its name -- the hooks of fieldops.hip switch on it and the tests' ids carry it -- so a signature that the
    committed file already holds keeps its place (the places of dropped ones close up), and new ones follow in sorted order."""
    have = set(sigs)
    kept = [s for s in old if s in have]
    seen = set(kept)
    return kept + [s for s in sigs if s not in seen]


def render(sigs) -> str:
    lines = [
        "// GENERATED by tools/lz29_inventory.py -- do not edit.  Every typed lazy operation (lz29.hpp LzOps) the product instantiates:",
        "// LZ29_SIG(index, field, op, arity, Ka, Va, Kb, Vb, Kc, Vc, Kd, Vd, Kr, Vr) -- operand types (K, V) of Lz<F, K, V>, unused",
        "// operands 0, 0; the result type last (0, 0: canonical wire words).  Sources: " + ", ".join(sources()) + ".",
    ]
    for i, (field, op, args, r) in enumerate(sigs):
        ops = list(args) + [(0, 0)] * (4 - len(args))
        flat = ", ".join(f"{k}, {v}" for k, v in ops)
        lines.append(f"LZ29_SIG({i}, {field}, {op}, {len(args)}, {flat}, {r[0]}, {r[1]})")
    return "\n".join(lines) + "\n"


def main(argv):
    text = render(keep_indices(collect(), committed()))
    if "--check" in argv:
        cur = open(OUT).read() if os.path.exists(OUT) else ""
        if cur != text:
            sys.stderr.write("lz29_sigs.inc is stale: run tools/lz29_inventory.py\n")
            return 1
        return 0
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{OUT}: {text.count('LZ29_SIG(') - 1} signatures")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
