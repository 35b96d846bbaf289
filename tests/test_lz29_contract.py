"""CPU checks of the lazy 29-bit-limb contracts: the committed inventory of typed signatures is the product's (regenerated from clang's
AST and diffed, as test_rust_shim.py does for the bindings), no type states a value the nine limbs cannot hold, and a bit-exact model
of the products' column loops is exact at the extremes of every inventoried product signature -- and wraps one step outside the limb
contract, so the inputs of tests/test_gpu_lz29_bounds.py reach the overflow that LzOps::cols_fit guards against."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lz29_contract as lc

ROOT = lc.ROOT


def test_inventory_is_current():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lz29_inventory.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr + res.stdout


def test_inventory_covers_the_typed_kernels():
    sigs = lc.signatures()
    assert [s["index"] for s in sigs] == list(range(len(sigs)))
    ops = {s["op"] for s in sigs}
    assert {"add", "sub", "mul", "mul2", "sqr", "norm", "to_wire", "canon", "assume"} <= ops, ops
    assert {s["field"] for s in sigs} == {"FQ", "FR"}


def test_no_type_exceeds_the_nine_limbs():
    """Lz<F, K, V> is storable only while V ((M >> 232) + 1) <= 2^32 (lz29.hpp value_fits): V <= 1354 for both fields."""
    for fld, mod in lc.MOD.items():
        assert (1 << 32) // ((mod >> 232) + 1) == 1354
    for s in lc.signatures():
        for k, v in s["args"] + ([s["res"]] if s["res"] else []):
            assert 1 <= k <= 7 and v * ((lc.MOD[s["field"]] >> 232) + 1) <= 1 << 32, s


def _extremes(k, v, mod):
    rng = np.random.default_rng(k * 1000 + v)
    return lc.gen_type(k, v, mod, rng, n_random=2)


@pytest.mark.parametrize("op", ["mul", "sqr", "mul2"])
def test_column_model_is_exact_on_every_inventoried_product(op):
    sigs = [s for s in lc.signatures() if s["op"] == op]
    assert sigs
    for s in sigs:
        fld, mod = s["field"], lc.MOD[s["field"]]
        ins = [_extremes(k, v, mod) for k, v in s["args"]]
        rk, rv = s["res"]
        for j in range(3):                                  # (a), (b), (c) on every operand at once, then mixed
            for sel in ([j] * len(ins), [(j + t) % 3 for t in range(len(ins))]):
                xs = [ins[t][sel[t]] for t in range(len(ins))]
                if op == "mul":
                    r, wrapped = lc.model_mul(xs[0], xs[1], fld)
                    want = lc.value(xs[0]) * lc.value(xs[1])
                elif op == "sqr":
                    r, wrapped = lc.model_sqr(xs[0], fld)
                    want = lc.value(xs[0]) ** 2
                else:
                    r, wrapped = lc.model_mul2(*xs, fld)
                    want = lc.value(xs[0]) * lc.value(xs[1]) + lc.value(xs[2]) * lc.value(xs[3])
                assert not wrapped, (s, sel)
                assert lc.value(r) % mod == lc.mont261(want, mod), (s, sel)
                lc.check_type(r, rk, rv, mod, f"{s}")
                assert all(x < lc.B for x in r[:8])


def test_column_model_wraps_one_step_outside_the_limb_contract():
    """Ka Kb = 9 (both operands' low limbs at 3 (2^29 + 2^6) - 1, the top limbs at their maximum for V = 32): lz29.hpp refuses the
    type (Ka Kb <= 6, cols_fit) and the model's accumulator does overflow."""
    for fld, mod in lc.MOD.items():
        a = lc.gen_type(3, 32, mod, np.random.default_rng(1), n_random=0)[0]
        assert not lc.cols_fit(3, 32, 3, 32)
        _, wrapped = lc.model_mul(a, a, fld)
        assert wrapped
        r, wrapped = lc.model_mul(a[:8] + [0], a[:8] + [0], fld)   # the same limbs without the top ones still overflow
        assert wrapped


def test_cols_fit_is_sound_against_the_model():
    """Wherever cols_fit (and the limb rule Ka Kb <= 6) admits a product, the model stays exact at the extreme inputs (a), (b)."""
    checked = 0
    for fld, mod in lc.MOD.items():
        for ka, kb in [(1, 1), (1, 2), (2, 2), (1, 3), (2, 3), (1, 6)]:
            for va in (1, 32, 169, 500, 1354):
                for vb in (1, 32, 169, 500, 1354):
                    if not lc.cols_fit(ka, va, kb, vb) or va * vb >= 169 * 512:
                        continue
                    xa, xb = _extremes(ka, va, mod), _extremes(kb, vb, mod)
                    for i in range(2):
                        for j in range(2):
                            _, wrapped = lc.model_mul(xa[i], xb[j], fld)
                            assert not wrapped, (fld, ka, va, kb, vb, i, j)
                            checked += 1
    assert checked > 50


def _model_reduce(a, fld):
    """fp29.hpp reduce(): norm, q = (l[8] MU) >> 32, a - q M."""
    c = lc.CONSTS[fld]
    v = lc.value(a)
    top = v >> 232
    q = (top * c["MU"]) >> 32
    return v - q * lc.MOD[fld]


def test_reduce_estimate_covers_32M():
    """reduce()'s quotient estimate from the top limb with MU = floor(2^264 / M): for values below 32 M (acc29_set passes it
    from_fp_x32 of a canonical coordinate, up to 32 (M - 1)) the remainder is in [0, 2 M) -- the argument fp29.hpp states."""
    for fld, mod in lc.MOD.items():
        assert lc.CONSTS[fld]["MU"] == (1 << 264) // mod
        for v in [32 * (mod - 1), 32 * mod - 1, 16 * mod, 16 * mod - 1, 2 * mod, mod, 0] + [k * mod + d for k in range(32) for d in (-1, 0, 1 << 232)]:
            if not 0 <= v < 32 * mod:
                continue
            r = _model_reduce(lc.limbs(v), fld)
            assert 0 <= r < 2 * mod, (fld, v // mod)


def _reaches_lz29(path, seen):
    """Does the file include lz29.hpp, directly or through the headers it includes?  (Quoted includes, resolved next to the includer.)"""
    path = os.path.normpath(path)
    if path in seen or not os.path.exists(path):
        return False
    seen.add(path)
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
        if os.path.basename(inc) == "lz29.hpp" or _reaches_lz29(os.path.join(os.path.dirname(path), inc), seen):
            return True
    return False


def test_inventory_sources_are_the_include_closure():
    """Every kernel file that reaches lz29.hpp through any chain of headers (g2msm.hip: g2_29.hpp -> fq2_29.hpp -> lz29.hpp) is a
    source of the committed inventory; fieldops.hip, the test hooks generated from it, is the one exception.  Computed here from the
    #include lines, not from the tool's own list."""
    reaching = sorted(n for n in os.listdir(lc.CSRC) if n.endswith(".hip") and _reaches_lz29(os.path.join(lc.CSRC, n), set()))
    assert "g2msm.hip" in reaching and "fieldops.hip" in reaching and "ntt.hip" not in reaching, reaching
    head = "".join(line for line in open(os.path.join(lc.CSRC, "lz29_sigs.inc")) if line.startswith("//"))
    named = re.search(r"Sources: ([^\n]*)\.\n", head).group(1).split(", ")
    assert "g2msm.hip" in named and "fieldops.hip" not in named, named
    missing = [n for n in reaching if n != "fieldops.hip" and n not in named]
    assert not missing, f"reach lz29.hpp but are not inventoried: {missing}"


def test_regenerating_keeps_the_indices_of_committed_signatures():
    """An entry's index names its hook in fieldops.hip and its GPU test: the tool keeps a committed signature in its place, closes up
    over dropped ones and appends new ones in sorted order; and the committed file is such a fixed point of its own order."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("lz29_inventory", os.path.join(ROOT, "tools", "lz29_inventory.py"))
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    a, b, c, d = (("FQ", "add", ((1, 2), (1, 2)), (2, 4)), ("FQ", "sub", ((1, 2), (1, 2)), (2, 4)),
                  ("FR", "mul", ((1, 2), (1, 2)), (1, 2)), ("FQ", "mul", ((1, 4), (1, 4)), (1, 2)))
    assert inv.keep_indices([a, b, c], []) == [a, b, c]
    assert inv.keep_indices([a, d, b, c], [c, a]) == [c, a, d, b]            # kept in the committed order, new ones after, sorted
    assert inv.keep_indices([a, d, c], [b, c, a]) == [c, a, d]               # a dropped entry closes up
    old = inv.committed()
    assert [(s["field"], s["op"], tuple(s["args"]), s["res"] or (0, 0)) for s in lc.signatures()] == old
    assert inv.keep_indices(sorted(old), old) == old
