"""The lazy 29-bit-limb contracts (uzkge_amd/csrc/fp29.hpp, lz29.hpp) as plain integer arithmetic: the constants, the inventory of
typed signatures (lz29_sigs.inc), inputs at the edges of a type, checks of a raw result against its contract, and a bit-exact model
of the C++ column loops of the products (64-bit accumulator, wrap-around included).  Test infrastructure: no GPU needed."""
import os
import re

import numpy as np

import bn254_py as opy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uzkge_amd", "csrc")
B = 1 << 29
MASK = B - 1
U64 = (1 << 64) - 1
MOD = {"FQ": opy.P, "FR": opy.R}
FIELD_ID = {"FQ": 0, "FR": 1}

# uzk_test_l29_kat opcodes (include/uzkge_gpu_test.h)
OP = dict(mul=0, sqr=1, mul2=2, mul_cpp=3, sqr_cpp=4, mul2_cpp=5, mulc=6, mulcs=7, add=8, norm=9, norm1=10, reduce=11, reduce3=12,
          canon=13, to_fp=14, to_fp_div5=15, to_fp_div10=16, sub4=17, sub8=18, sub12=19, sub_off=20, sig=21, reduce_x32=22)
OFF_NAMES = ("OFF4", "OFF8", "OFF12", "OFF4T3", "OFF2T1", "OFF8T1")


def _consts():
    text = open(os.path.join(CSRC, "fp29_consts.inc")).read()
    out = {}
    for fld, body in re.findall(r"struct (Fq|Fr)29Cfg \{(.*?)\n\};", text, re.S):
        c = {}
        for name, vals in re.findall(r"uint32_t (\w+)\[9\] = \{([^}]*)\}", body):
            c[name] = [int(v.strip().rstrip("u"), 16) for v in vals.split(",")]
        for name, val in re.findall(r"uint32_t (\w+) = (0x[0-9a-f]+)u;", body):
            c[name] = int(val, 16)
        out[fld.upper()] = c
    return out


CONSTS = _consts()


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def limbs(x):
    """Normalized 9-limb digits of x (top limb: the rest; x < 2^264)."""
    assert 0 <= x < 1 << 264
    return [(x >> (29 * i)) & MASK for i in range(8)] + [x >> 232]


def from_fp_x32(words_value):
    """fp29.hpp from_fp_x32: the 256-bit word value re-limbed at offset -5 (= 32 x, normalized limbs)."""
    return limbs(words_value << 5)


# ---- the inventory ---------------------------------------------------------------------------------------------------------------
def signatures():
    """Every LZ29_SIG of lz29_sigs.inc: dict(index, field, op, args=[(K, V), ...], res=(K, V) or None for wire words)."""
    out = []
    for line in open(os.path.join(CSRC, "lz29_sigs.inc")):
        if not line.startswith("LZ29_SIG("):
            continue
        f = [t.strip() for t in line[len("LZ29_SIG("):line.rindex(")")].split(",")]
        idx, fld, op, ar = int(f[0]), f[1], f[2], int(f[3])
        nums = [int(t) for t in f[4:]]
        args = [(nums[2 * i], nums[2 * i + 1]) for i in range(ar)]
        res = None if (nums[8], nums[9]) == (0, 0) else (nums[8], nums[9])
        out.append(dict(index=idx, field=fld, op=op, args=args, res=res))
    return out


def prod_v(va, vb):
    return 1 + (va * vb + 168) // 169


def kt(v):
    return 1 + v // 169


def cols_fit(ka, va, kb, vb):
    """lz29.hpp LzOps::cols_fit, restated."""
    ta, tb = max(kt(va), ka), max(kt(vb), kb)
    return ta * kb + tb * ka + 7 * ka * kb + 9 < 64


# ---- inputs at the edges of a type -------------------------------------------------------------------------------------------------
def low_max(k):
    return k * (B + 64) - 1


def gen_type(k, v, mod, rng, n_random=8):
    """Limb vectors of type Lz<F, k, v> (every low limb < k (2^29 + 2^6), value < v M): (a) every low limb at its maximum and the
    largest top limb that keeps the value in range, (b) low limbs 0 and the top limb at its maximum, (c) v M - 1 in plain digits,
    (d) random limbs within the bound, (e) 0, 1 and small values."""
    top_of = lambda low: (v * mod - 1 - value(low + [0])) >> 232
    hi = low_max(k)
    out = []
    low = [hi] * 8
    out.append(low + [top_of(low)])                                   # (a)
    out.append([0] * 8 + [top_of([0] * 8)])                           # (b)
    out.append(limbs(v * mod - 1))                                    # (c)
    for _ in range(n_random):                                         # (d)
        low = [int(x) for x in rng.integers(0, hi + 1, size=8)]
        out.append(low + [int(rng.integers(0, top_of(low) + 1))])
    for small in (0, 1, 2, mod - 1):                                  # (e)
        if small < v * mod:
            out.append(limbs(small))
    for x in out:
        assert in_type(x, k, v, mod), (k, v, x)
    return out


def in_type(l, k, v, mod):
    return all(0 <= x < k * (B + 64) for x in l[:8]) and 0 <= l[8] < 1 << 32 and value(l) < v * mod


def pairs(xs, ys, rng, n_random=16):
    """Every pair of the first three (extreme) inputs of each side, plus random pairs."""
    out = [(a, b) for a in xs[:3] for b in ys[:3]]
    for _ in range(n_random):
        out.append((xs[int(rng.integers(len(xs)))], ys[int(rng.integers(len(ys)))]))
    return out


# ---- results against their contracts -----------------------------------------------------------------------------------------------
def mont261(x, mod):
    return x * pow(2, -261, mod) % mod


def check_type(r, k, v, mod, what=""):
    assert in_type(r, k, v, mod), f"{what}: result {r} (value {value(r) / mod:.3f} M) outside Lz<{k}, {v}>"


def check_normalized(r, vmax_num, vmax_den, mod, what=""):
    """Low limbs < 2^29, value < M * vmax_num / vmax_den."""
    assert all(x < B for x in r[:8]), f"{what}: limbs not normalized {r}"
    assert value(r) * vmax_den < mod * vmax_num, f"{what}: value {value(r) / mod:.3f} M over {vmax_num}/{vmax_den} M"


# ---- the products' column loops, bit-exact (fp29.hpp mul_cpp / sqr_cpp / mul2_cpp) ---------------------------------------------------
def _mont_columns(pairs_of_col, fld):
    """The shared column loop: pairs_of_col(k) lists the operand products of column k (k < 17).  Returns (limbs, wrapped): the
    64-bit model's result and whether any accumulation wrapped (an exact result then would differ)."""
    c = CONSTS[fld]
    M, INV = c["M"], c["INV"]
    acc, wrapped, m, r = 0, False, [0] * 9, [0] * 9

    def add(x):
        nonlocal acc, wrapped
        acc += x
        if acc > U64:
            wrapped = True
            acc &= U64

    for k in range(9):
        for x in pairs_of_col(k):
            add(x)
        for i in range(k):
            add(m[i] * M[k - i])
        m[k] = ((acc & 0xFFFFFFFF) * INV) & 0xFFFFFFFF & MASK
        add(m[k] * M[0])
        acc >>= 29
    for k in range(9, 17):
        for x in pairs_of_col(k):
            add(x)
        for i in range(k - 8, 9):
            add(m[i] * M[k - i])
        r[k - 9] = acc & 0xFFFFFFFF & MASK
        acc >>= 29
    r[8] = acc & 0xFFFFFFFF
    return r, wrapped


def _cols(a, b):
    return lambda k: [a[i] * b[k - i] for i in range(max(0, k - 8), min(k, 8) + 1)]


def model_mul(a, b, fld):
    return _mont_columns(_cols(a, b), fld)


def model_sqr(a, fld):
    d = [(x << 1) & 0xFFFFFFFF for x in a]

    def col(k):
        lo = max(0, k - 8)
        out = [a[i] * d[k - i] for i in range(lo, 9) if 2 * i < k]
        if k % 2 == 0:
            out.append(a[k // 2] * a[k // 2])
        return out
    return _mont_columns(col, fld)


def model_mul2(a, b, c, d, fld):
    f, g = _cols(a, b), _cols(c, d)
    return _mont_columns(lambda k: f(k) + g(k), fld)


# ---- numpy plumbing for the hooks -------------------------------------------------------------------------------------------------
def records(rows):
    """[[a, b, c, d], ...] of limb lists (missing operands: zeros) -> (n, 4, 9) uint32."""
    out = np.zeros((len(rows), 4, 9), dtype=np.uint32)
    for i, ops in enumerate(rows):
        for j, l in enumerate(ops):
            out[i, j] = l
    return out


def words_value(r):
    """An 8-word result (l[0..7] = 32-bit words) -> its integer."""
    assert int(r[8]) == 0
    return sum(int(x) << (32 * i) for i, x in enumerate(r[:8]))
