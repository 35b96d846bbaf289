"""The lazy 29-bit-limb primitives (fp29.hpp) and typed operations (lz29.hpp) on RAW limbs at the edges of their contracts
(uzk_test_l29_kat: no re-limbing on the way in, no canon on the way out).  Every inventoried signature (lz29_sigs.inc) in its field
gets inputs at its type's extremes plus random ones; each raw result must have the right residue AND meet the bound its type or
fp29.hpp's header states -- the next operation relies on that bound, which a canon()ed known answer never shows.  Then the
primitives at the ranges their callers use (ntt.hip's radix-4 outputs into mulc / reduce, acc29_set's reduce of up to 32 (M - 1)),
and ec29l.hpp's additions with every coordinate at its largest representative below 32 M."""
import ctypes
import zlib

import numpy as np
import pytest

import bn254_py as opy
import lz29_contract as lc
from lz29_contract import B, OP, limbs, value

pytestmark = pytest.mark.gpu


def _run(field, op, rows, param=0):
    from uzkge_amd import _native as N
    from uzkge_amd.backend import check
    x = lc.records(rows)
    out = np.zeros((len(rows), 9), dtype=np.uint32)
    check(N.lib.uzk_test_l29_kat(lc.FIELD_ID[field], op, param, x.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), len(rows)))
    return [[int(v) for v in r] for r in out]


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


SIGS = lc.signatures()


def _inputs(s, n_random=200):
    mod = lc.MOD[s["field"]]
    rng = _rng(s["index"])
    ins = [lc.gen_type(k, v, mod, rng, n_random=12) for k, v in s["args"]]
    if len(ins) == 1:
        rows = [[a] for a in ins[0]]
    elif len(ins) == 2:
        rows = [list(p) for p in lc.pairs(ins[0], ins[1], rng, n_random=n_random)]
    else:
        rows = [[ins[t][j] for t in range(4)] for j in range(3)]
        rows += [[ins[t][(j + t) % 3] for t in range(4)] for j in range(3)]
        rows += [[ins[t][int(rng.integers(len(ins[t])))] for t in range(4)] for _ in range(n_random)]
    return rows


@pytest.mark.parametrize("s", [s for s in SIGS if s["op"] != "assume"], ids=lambda s: f"{s['index']}-{s['field']}-{s['op']}")
def test_inventoried_signature_meets_its_contract(gpu, s):
    fld, mod = s["field"], lc.MOD[s["field"]]
    rows = _inputs(s)
    op = s["op"]
    if op in ("sub", "to_wire", "canon"):
        got = _run(fld, OP["sig"], rows, s["index"])
    elif op in ("mul", "sqr", "mul2"):
        got = _run(fld, OP[op], rows)
        assert got == _run(fld, OP[op + "_cpp"], rows), "assembly and C++ products differ"
    elif op == "add":
        got = _run(fld, OP["add"], rows)
    else:
        got = _run(fld, OP["norm1"], rows)                   # LzOps::norm is one parallel carry step
    for ops, r in zip(rows, got):
        v = [value(x) for x in ops]
        if op == "sub":
            want = (v[0] - v[1]) % mod
        elif op == "add":
            want = (v[0] + v[1]) % mod
        elif op == "mul":
            want = lc.mont261(v[0] * v[1], mod)
        elif op == "sqr":
            want = lc.mont261(v[0] * v[0], mod)
        elif op == "mul2":
            want = lc.mont261(v[0] * v[1] + v[2] * v[3], mod)
        else:
            want = v[0] % mod
        if op == "to_wire":                                  # x 2^261 -> canonical x 2^256
            w = lc.words_value(r)
            assert w == v[0] * pow(32, -1, mod) % mod, (s, ops)
        elif op == "canon":
            assert lc.words_value(r) == v[0] % mod, (s, ops)
        else:
            assert value(r) % mod == want, (s, ops, r)
            lc.check_type(r, *s["res"], mod, what=str(s))
            if op in ("mul", "sqr", "mul2"):
                assert all(x < B for x in r[:8]), (s, r)


@pytest.mark.parametrize("fld", ["FQ", "FR"])
def test_sub_offsets_never_underflow(gpu, fld):
    """sub<4 | 8 | 12> and sub_off with every named offset k M, subtrahends at the limb bounds fp29.hpp states for each and values up
    to (k - 1) M (the pre-borrow takes up to 2 from the offset's top limb; lz29.hpp's Off29 keeps the same margin): the raw result is
    exactly a - b + OFF limb by limb (no limb wrapped) and congruent to a - b."""
    mod, c = lc.MOD[fld], lc.CONSTS[fld]
    rng = _rng("sub", fld)
    a_in = lc.gen_type(1, 1, mod, rng, n_random=8)
    # (offset name, opcode, param, limb bound of b, value bound of b in M)
    cases = [("OFF4", OP["sub4"], 0, 2 * B, 4), ("OFF8", OP["sub8"], 0, 2 * B, 8), ("OFF12", OP["sub12"], 0, 2 * B, 12)]
    cases += [(name, OP["sub_off"], i, {"OFF4T3": 3 * B - 2, "OFF2T1": B, "OFF8T1": B}.get(name, 2 * B), int(name[3:].split("T")[0]))
              for i, name in enumerate(lc.OFF_NAMES)]
    for name, op, param, lb, vk in cases:
        vb = (vk - 1) * mod
        top = (vb - 1 - value([lb - 1] * 8 + [0])) >> 232
        bs = [[lb - 1] * 8 + [top], limbs(vb - 1), [0] * 8 + [(vb - 1) >> 232], [0] * 9, limbs(1)]
        bs = [b for b in bs if value(b) < vb and all(x < lb for x in b[:8])]
        assert len(bs) == 5, name
        rows = [[a, b] for a in a_in for b in bs]
        got = _run(fld, op, rows, param)
        off = c[name]
        for (a, b), r in zip(rows, got):
            exact = [a[i] - b[i] + off[i] for i in range(9)]
            assert all(0 <= e < 1 << 32 for e in exact), (name, a, b)
            assert r == exact and value(r) % mod == (value(a) - value(b)) % mod, (name, a, b)


@pytest.mark.parametrize("fld", ["FQ", "FR"])
def test_reduce_canon_norm_at_their_ranges(gpu, fld):
    """reduce: limbs < 2^32 - 2^3, value < 32 M (the documented 16 M and acc29_set's from_fp_x32 range) -> normalized, < 2 M;
    reduce3: limbs < 2^31.5, value < 16 M -> normalized, < 3 M; canon: < 16 M -> [0, M); norm (limbs < 2^32 - 2^3) / norm1 (limbs
    < 2^32): value kept, limbs < 2^29 / < 2^29 + 2^3."""
    mod = lc.MOD[fld]
    rng = _rng("reduce", fld)
    lim32, lim315 = (1 << 32) - 8, int(2 ** 31.5)

    def ranged(limb_lim, vmax, n=150):
        out = []
        for v in (vmax, vmax // 2, 17, 16, 3, 2, 1):
            top = (v * mod - 1 - value([limb_lim - 1] * 8 + [0])) >> 232
            if top >= 0:
                out.append([limb_lim - 1] * 8 + [top])
            out.append(limbs(v * mod - 1))
            out.append([0] * 8 + [(v * mod - 1) >> 232])
        for _ in range(n):
            low = [int(x) for x in rng.integers(0, limb_lim, size=8)]
            top_max = (vmax * mod - 1 - value(low + [0])) >> 232
            out.append(low + [int(rng.integers(0, top_max + 1))])
        return [x for x in out if value(x) < vmax * mod and max(x[:8]) < limb_lim]

    xs = ranged(lim32, 32)
    for x, r in zip(xs, _run(fld, OP["reduce"], [[x] for x in xs])):
        assert value(r) % mod == value(x) % mod
        lc.check_normalized(r, 2, 1, mod, f"reduce({value(x) / mod:.2f} M)")
    # what acc29_set does: from_fp_x32 of the canonical words of a coordinate, up to M - 1
    ws = [mod - 1, mod - 2, (1 << 253) + 12345, 1, 0] + [int(rng.integers(0, 1 << 62)) * (mod >> 62) % mod for _ in range(64)]
    rows = [[[(w >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0]] for w in ws]
    for w, r in zip(ws, _run(fld, OP["reduce_x32"], rows)):
        assert value(r) % mod == 32 * w % mod
        lc.check_normalized(r, 2, 1, mod, f"reduce(from_fp_x32({w}))")
    xs = ranged(lim315, 16)
    for x, r in zip(xs, _run(fld, OP["reduce3"], [[x] for x in xs])):
        assert value(r) % mod == value(x) % mod
        lc.check_normalized(r, 3, 1, mod, "reduce3")
    xs = ranged(lim32, 16)
    for x, r in zip(xs, _run(fld, OP["canon"], [[x] for x in xs])):
        assert value(r) == value(x) % mod and all(l < B for l in r[:8]), "canon"
    xs = ranged(lim32, 32)                                   # norm: the carry (< 2^3) joins the next limb before it is split
    for x, r in zip(xs, _run(fld, OP["norm"], [[x] for x in xs])):
        assert value(r) == value(x) and all(l < B for l in r[:8]), "norm"
    xs = ranged(1 << 32, 32)
    for x, r in zip(xs, _run(fld, OP["norm1"], [[x] for x in xs])):
        assert value(r) == value(x) and all(l < B + 8 for l in r[:8]), "norm1"


@pytest.mark.parametrize("fld", ["FQ", "FR"])
def test_mulc_and_conversions_at_their_ranges(gpu, fld):
    """mulc / mulcs: x with limbs < 2^31.5 and value < 10 M (ntt.hip's radix-4 outputs; and value < 2^261) times a canonical w ->
    normalized, < 3 M, = x w mod M; the uniform form agrees with the per-lane one.  to_fp: normalized limbs, value < 2^256 -> its
    words; to_fp_div<S>: limbs < 2^32, value < V M with V <= 2^S and V + 2^S <= 1354 (a + k M fits the nine limbs) -> a 2^-S mod M,
    < 2 M."""
    mod = lc.MOD[fld]
    rng = _rng("mulc", fld)
    lim = int(2 ** 31.5)
    xs = []
    for vm in (10, 1):
        top = (vm * mod - 1 - value([lim - 1] * 8 + [0])) >> 232
        xs += [[lim - 1] * 8 + [top], limbs(vm * mod - 1), [0] * 8 + [(vm * mod - 1) >> 232]]
    xs += [[int(x) for x in rng.integers(0, lim, size=8)] + [int(rng.integers(0, 1 << 20))] for _ in range(200)]
    xs += [limbs((1 << 261) - 1 - i) for i in range(2)] if (1 << 261) - 1 < 1 << 264 else []
    xs = [x for x in xs if max(x[:8]) < lim and value(x) < 1 << 261]
    for w in (mod - 1, 1, 0, int(rng.integers(0, 1 << 62)) * (mod >> 62) % mod):
        rows = [[x, limbs(w)] for x in xs]
        got, gots = _run(fld, OP["mulc"], rows), _run(fld, OP["mulcs"], rows)
        assert got == gots, "mulcs differs from mulc"
        for x, r in zip(xs, got):
            assert value(r) % mod == value(x) * w % mod
            lc.check_normalized(r, 3, 1, mod, "mulc")
    ns = [limbs(x) for x in ((1 << 256) - 1, mod - 1, 0, 1, 1 << 255)] + [limbs(int(rng.integers(0, 1 << 62)) << 190) for _ in range(16)]
    for x, r in zip(ns, _run(fld, OP["to_fp"], [[x] for x in ns])):
        assert lc.words_value(r) == value(x)
    for s, opc in ((5, OP["to_fp_div5"]), (10, OP["to_fp_div10"])):
        ys = lc.gen_type(6, min(1 << s, 1354 - (1 << s)), mod, rng, n_random=64)
        for y, r in zip(ys, _run(fld, opc, [[y] for y in ys])):
            w = lc.words_value(r)
            assert w < 2 * mod and w % mod == value(y) * pow(2, -s, mod) % mod, (s, y)


# ---- ec29l.hpp additions at the lazy extremes -------------------------------------------------------------------------------------
def _xyzz_261(pt, z):
    """An affine point as XYZZ (x z^2, y z^3, z^2, z^3) in the 2^261-form, each coordinate its largest representative below 32 M."""
    p = opy.P
    x, y = pt
    zz, zzz = z * z % p, z * z * z % p
    out = []
    for c in (x * zz % p, y * zzz % p, zz, zzz):
        m = c * (1 << 261) % p
        m += (32 * p - 1 - m) // p * p
        out.append(_raise_low(limbs(m)))
    return out


def _raise_low(l):
    """Raise a low limb by 2^29 (borrowing one from the limb above) wherever the result stays < 2^29 + 2^6: same value."""
    l = list(l)
    for i in range(8):
        if l[i] < 64 and l[i + 1] >= 1:
            l[i] += B
            l[i + 1] -= 1
    return l


def _affine_of(coords):
    p = opy.P
    X, Y, ZZ, ZZZ = (value(c) * pow(2, -261, p) % p for c in coords)
    if ZZ == 0:
        return None
    return (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p)


@pytest.mark.parametrize("op", [0, 1, 2, 3], ids=["add", "dbl", "add_quad", "dbl_quad"])
def test_p29_additions_at_the_lazy_extremes(gpu, op):
    from uzkge_amd import _native as N
    from uzkge_amd.backend import check
    rng = _rng("p29", op)
    g = opy.G1_GEN
    n = 48
    rows = np.zeros((n, 2, 4, 9), dtype=np.uint32)
    want = []
    for i in range(n):
        a = opy.g1_mul(g, int(rng.integers(1, 1 << 62)))
        b = a if i % 8 == 7 else opy.g1_mul(g, int(rng.integers(1, 1 << 62)))       # equal points: the doubling branch
        za, zb = (1, 1) if i == 0 else (int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 62)))
        rows[i, 0] = _xyzz_261(a, za)
        rows[i, 1] = _xyzz_261(b, zb)
        want.append(opy.g1_add(a, b) if op in (0, 2) else opy.g1_add(a, a))
    out = np.zeros((n, 4, 9), dtype=np.uint32)
    check(N.lib.uzk_test_p29_kat(op, rows.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), n))
    for i in range(n):
        coords = [[int(v) for v in out[i, c]] for c in range(4)]
        for c in coords:
            lc.check_type(c, 1, 32, opy.P, f"p29 op {op} coordinate")
        assert _affine_of(coords) == want[i], i
