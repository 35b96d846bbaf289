"""Shared inputs of the pairing tests: the wire forms of Fq12 elements and of pairs of points, pairs of known discrete logarithm
(P_i = a_i G through the fixed-base tables of g16_ref, Q_i = (i + 1) H by repeated addition, as tests/g2_cases.py builds its column)
and the closed form of their product, e(G, H)^(sum a_i (i + 1) mod r): one oracle pairing and one f12_pow for any number of pairs."""
import random
import re
import os

import numpy as np

import bn254_pairing as op
import bn254_py as opy
import g16_ref as gr
import g2_ref as g2

P, R = op.P, op.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = [(1, 0)] + [(0, 0)] * 5


def header_constant(name, header="uzkge_gpu.h"):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(os.path.join(ROOT, "include", header)).read()).group(1))


def gt_to_wire(elems):
    """[n, 6, 2, 4] uint64 from a list of Fq12 elements (six Fq2 pairs of integers)"""
    out = np.zeros((len(elems), 6, 2, 4), dtype=np.uint64)
    for i, e in enumerate(elems):
        for k in range(6):
            out[i, k] = np.asarray(g2.fq2_to_wire(e[k]), dtype=np.uint64).reshape(2, 4)
    return out


def gt_from_wire(w):
    w = np.asarray(w, dtype=np.uint64).reshape(-1, 6, 2, 4)
    return [[tuple(int(v) for v in g2.fq2_from_wire(row[k].reshape(8))) for k in range(6)] for row in w]


def rand_f12(rng):
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]


def edge_f12():
    """every coefficient 0, 1 and p - 1 in every position; zero; one; a single w^k"""
    out = [[(0, 0)] * 6, list(ONE), [(1, 1)] * 6, [(P - 1, P - 1)] * 6, [(P - 1, 0), (0, P - 1)] * 3, [(0, 1), (P - 1, 1)] * 3]
    for k in range(6):
        out.append([(P - 1, 1) if j == k else (0, 0) for j in range(6)])
    return out


def p_wire(points):
    return gr.g1_to_wire(points) if points else np.zeros((0, 8), dtype=np.uint64)


def q_wire(points):
    return g2.points_to_wire(points) if points else np.zeros((0, 16), dtype=np.uint64)


_cache = {}


def h_multiples(n):
    """[H, 2 H, .., n H] by repeated addition"""
    have = _cache.setdefault("h", [])
    while len(have) < n:
        have.append(op.g2_add(have[-1], op.G2_GEN) if have else op.G2_GEN)
    return have[:n]


def e_gh():
    if "e" not in _cache:
        _cache["e"] = op.pairing(opy.G1_GEN, op.G2_GEN)
    return _cache["e"]


def logs_of(n, seed, total=None):
    rng = random.Random(f"pairing-logs-{n}-{seed}")
    a = [rng.randrange(1, R) for _ in range(n)]
    if total is not None:
        rest = sum(x * (i + 1) for i, x in enumerate(a[:-1])) % R
        a[-1] = (total - rest) * pow(n, R - 2, R) % R
    return a


def log_pairs(n, seed, total=None):
    """(p [n, 8], q [n, 16], s): n pairs (a_i G, (i + 1) H) as wire points -- a_i G through the C oracle -- and s = sum a_i (i + 1)
    mod r; with `total` given, the last a is chosen so that s = total (n >= 1)"""
    import oracle_c as oc
    a = logs_of(n, seed, total)
    s = sum(x * (i + 1) for i, x in enumerate(a)) % R
    gen = oc.points_from_affine([opy.G1_GEN]).reshape(8)
    sc = oc.fr_from_ints(a).reshape(-1, 4) if n else np.zeros((0, 4), dtype=np.uint64)
    p = np.zeros((n, 8), dtype=np.uint64)
    for i in range(n):
        p[i] = oc.g1_to_affine(oc.g1_mul(gen, sc[i])) if a[i] else 0
    return p, q_wire(h_multiples(n)), s


def expected_power(s):
    return op.f12_pow(e_gh(), s) if s % R else list(ONE)
