"""CPU reference for the G2 MSM, Python integers only: decompression of the Groth16 fixture's two columns, a Jacobian signed-window
Pippenger over Fq2, and the wire format of include/uzkge_gpu.h (c0 then c1, 4 x u64 LE Montgomery words each).

Points are affine tuples ((x0, x1), (y0, y1)) of plain integers, None = infinity -- the convention of oracle/bn254_pairing.py, whose
g2_add / g2_mul are the naive oracle this module's Pippenger is held to (tests/test_g2_ref_host.py)."""
import os
import struct

import numpy as np

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "groth16-reveal-b-queries.bin")
FIXTURE_SHA256 = "a5d599740b8d7c8ee3c2bf5ab8e566be8d48ae1b838ed1a10cdf17b3de219bbd"
N_QUERY = 4869

# twist: y^2 = x^3 + 3 / (9 + u)
_d = pow(82, P - 2, P)
B2 = (27 * _d % P, (-3 * _d) % P)


# ---- Fq, Fq2 ----
def fq_sqrt(a):
    """square root in Fq (p = 3 mod 4), or None"""
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


def f2_add(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
def f2_sub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
def f2_neg(a): return ((-a[0]) % P, (-a[1]) % P)
def f2_mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
def f2_sqr(a): return ((a[0] + a[1]) * (a[0] - a[1]) % P, 2 * a[0] * a[1] % P)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * n % P, (-a[1]) * n % P)


def f2_sqrt(a):
    """square root in Fq2 by the norm method, or None: with n = sqrt(a0^2 + a1^2), x0^2 = (a0 +- n) / 2 and x1 = a1 / (2 x0)"""
    if a[1] == 0:
        r = fq_sqrt(a[0])
        if r is not None:
            return (r, 0)
        r = fq_sqrt((-a[0]) % P)                      # u^2 = -1: sqrt(a0) = u sqrt(-a0)
        return None if r is None else (0, r)
    n = fq_sqrt((a[0] * a[0] + a[1] * a[1]) % P)
    if n is None:
        return None
    half = (P + 1) // 2
    for s in (n, P - n):
        x0 = fq_sqrt((a[0] + s) * half % P)
        if x0 is not None and x0 != 0:
            x = (x0, a[1] * pow(2 * x0, P - 2, P) % P)
            if f2_sqr(x) == (a[0] % P, a[1] % P):
                return x
    return None


def f2_gt(a, b):
    """ark-ff's ordering of Fq2: c1 first, then c0"""
    return (a[1], a[0]) > (b[1], b[0])


# ---- decompression (ark-serialize, compressed; flags in the top two bits of the last byte) ----
def decompress_g1(b):
    flags = b[31]
    if flags & 0x40:
        return None
    x = int.from_bytes(b[:31] + bytes([flags & 0x3f]), "little")
    y = fq_sqrt((x * x * x + 3) % P)
    assert y is not None
    if (y > P - y) != bool(flags & 0x80):
        y = P - y
    return (x, y)


def decompress_g2(b):
    flags = b[63]
    if flags & 0x40:
        return None
    x = (int.from_bytes(b[:32], "little"), int.from_bytes(b[32:63] + bytes([flags & 0x3f]), "little"))
    y = f2_sqrt(f2_add(f2_mul(f2_sqr(x), x), B2))
    assert y is not None
    if f2_gt(y, f2_neg(y)) != bool(flags & 0x80):
        y = f2_neg(y)
    return (x, y)


def g2_on_curve(q):
    return q is None or f2_sqr(q[1]) == f2_add(f2_mul(f2_sqr(q[0]), q[0]), B2)


_cache = {}


def load_fixture():
    """(b_g1_query, b_g2_query): 4869 affine points each (None = infinity)"""
    if "cols" not in _cache:
        data = open(FIXTURE, "rb").read()
        n1 = struct.unpack_from("<Q", data, 0)[0]
        g1 = [decompress_g1(data[8 + 32 * i:8 + 32 * (i + 1)]) for i in range(n1)]
        off = 8 + 32 * n1
        n2 = struct.unpack_from("<Q", data, off)[0]
        g2 = [decompress_g2(data[off + 8 + 64 * i:off + 8 + 64 * (i + 1)]) for i in range(n2)]
        _cache["cols"] = (g1, g2)
    return _cache["cols"]


# ---- Jacobian arithmetic over Fq2 (None = infinity) ----
def jac_dbl(p):
    if p is None:
        return None
    X, Y, Z = p
    A, B = f2_sqr(X), f2_sqr(Y)
    C = f2_sqr(B)
    D = f2_sub(f2_sub(f2_sqr(f2_add(X, B)), A), C)
    D = f2_add(D, D)
    E = f2_add(f2_add(A, A), A)
    X3 = f2_sub(f2_sqr(E), f2_add(D, D))
    C8 = f2_add(C, C); C8 = f2_add(C8, C8); C8 = f2_add(C8, C8)
    Y3 = f2_sub(f2_mul(E, f2_sub(D, X3)), C8)
    Z3 = f2_mul(Y, Z); Z3 = f2_add(Z3, Z3)
    return (X3, Y3, Z3)


def jac_madd(p, q):
    """p (Jacobian) + q (affine), complete"""
    if q is None:
        return p
    if p is None:
        return (q[0], q[1], (1, 0))
    X1, Y1, Z1 = p
    Z1Z1 = f2_sqr(Z1)
    U2, S2 = f2_mul(q[0], Z1Z1), f2_mul(q[1], f2_mul(Z1, Z1Z1))
    H, r = f2_sub(U2, X1), f2_sub(S2, Y1)
    if H == (0, 0):
        return jac_dbl(p) if r == (0, 0) else None
    HH = f2_sqr(H)
    HHH, V = f2_mul(H, HH), f2_mul(X1, HH)
    X3 = f2_sub(f2_sub(f2_sqr(r), HHH), f2_add(V, V))
    Y3 = f2_sub(f2_mul(r, f2_sub(V, X3)), f2_mul(Y1, HHH))
    return (X3, Y3, f2_mul(Z1, H))


def jac_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    Z1Z1, Z2Z2 = f2_sqr(Z1), f2_sqr(Z2)
    U1, U2 = f2_mul(X1, Z2Z2), f2_mul(X2, Z1Z1)
    S1, S2 = f2_mul(Y1, f2_mul(Z2, Z2Z2)), f2_mul(Y2, f2_mul(Z1, Z1Z1))
    H, r = f2_sub(U2, U1), f2_sub(S2, S1)
    if H == (0, 0):
        return jac_dbl(p) if r == (0, 0) else None
    HH = f2_sqr(H)
    HHH, V = f2_mul(H, HH), f2_mul(U1, HH)
    X3 = f2_sub(f2_sub(f2_sqr(r), HHH), f2_add(V, V))
    Y3 = f2_sub(f2_mul(r, f2_sub(V, X3)), f2_mul(S1, HHH))
    return (X3, Y3, f2_mul(f2_mul(Z1, Z2), H))


def jac_to_affine(p):
    if p is None or p[2] == (0, 0):
        return None
    zi = f2_inv(p[2])
    zi2 = f2_sqr(zi)
    return (f2_mul(p[0], zi2), f2_mul(p[1], f2_mul(zi2, zi)))


def g2_neg(q):
    return None if q is None else (q[0], f2_neg(q[1]))


def msm(points, scalars, c=8):
    """sum_i scalars[i] * points[i] (affine, None = infinity) by a signed-window Pippenger"""
    assert len(points) == len(scalars)
    half = 1 << (c - 1)
    windows = (254 + c - 1) // c + 1
    buckets = [[None] * (half + 1) for _ in range(windows)]
    for pt, s in zip(points, scalars):
        s %= R
        if pt is None or s == 0:
            continue
        npt = None
        w = 0
        while s:
            d = s & ((1 << c) - 1)
            s >>= c
            if d > half:
                d -= 1 << c
                s += 1
            if d > 0:
                buckets[w][d] = jac_madd(buckets[w][d], pt)
            elif d < 0:
                if npt is None:
                    npt = g2_neg(pt)
                buckets[w][-d] = jac_madd(buckets[w][-d], npt)
            w += 1
    total = None
    for w in range(windows - 1, -1, -1):
        for _ in range(c):
            total = jac_dbl(total)
        run = acc = None
        for k in range(half, 0, -1):
            run = jac_add(run, buckets[w][k])
            acc = jac_add(acc, run)
        total = jac_add(total, acc)
    return jac_to_affine(total)


# ---- wire format ----
def _fq_words(v):
    m = v * MONT % P
    return [(m >> (64 * k)) & 0xffffffffffffffff for k in range(4)]


def _fq_from_words(w):
    m = sum(int(w[k]) << (64 * k) for k in range(4))
    return m * pow(MONT, P - 2, P) % P


def fq2_to_wire(a):
    return np.array(_fq_words(a[0]) + _fq_words(a[1]), dtype=np.uint64)


def fq2_from_wire(w):
    return (_fq_from_words(w[0:4]), _fq_from_words(w[4:8]))


def points_to_wire(points):
    """(n, 16) uint64: x.c0, x.c1, y.c0, y.c1; infinity = zeros"""
    out = np.zeros((len(points), 16), dtype=np.uint64)
    for i, q in enumerate(points):
        if q is not None:
            out[i, 0:8] = fq2_to_wire(q[0])
            out[i, 8:16] = fq2_to_wire(q[1])
    return out


def point_from_wire(w):
    w = np.asarray(w).reshape(16)
    if not w.any():
        return None
    return (fq2_from_wire(w[0:8]), fq2_from_wire(w[8:16]))


def jac_to_wire(p):
    """(24,) uint64 Jacobian point of integers (X, Y, Z), None -> (1, 1, 0)"""
    if p is None:
        p = ((1, 0), (1, 0), (0, 0))
    return np.concatenate([fq2_to_wire(p[0]), fq2_to_wire(p[1]), fq2_to_wire(p[2])])


def scalars_to_wire(scalars):
    """(n, 4) uint64: Fr elements in Montgomery form"""
    out = np.zeros((len(scalars), 4), dtype=np.uint64)
    for i, s in enumerate(scalars):
        m = (s % R) * MONT % R
        for k in range(4):
            out[i, k] = (m >> (64 * k)) & 0xffffffffffffffff
    return out
