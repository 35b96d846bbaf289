"""The cases of tests/golden/vectors_g2.npz: one definition for the script that freezes the expected outputs
(tests/golden/make_vectors_g2.py), the CPU test that holds g2_ref to them and the GPU tests that hold the library to them."""
import random

import g2_ref as g

SIZES = (0, 1, 2, 33, 255, 256, 257, 1024, 4869)
CLASSES = ("uniform", "zero", "one", "rm1", "bool")
OFFSET_CASE = (1000, 500)                 # offset, n
INF_RANGE = (4862, 3)                     # the longest all-infinity range of the column: offset, n

# limb boundaries of both representations: 29-bit limbs (device) and 64-bit words (wire)
_EDGE_FQ = (0, 1, g.P - 1, g.P - 2, (1 << 29) - 1, 1 << 29, (1 << 64) - 1, 1 << 64, (1 << 232) - 1, 1 << 232, (1 << 253) + 5, (g.P - 1) // 2)


def scalars(cls, n, seed=0):
    rng = random.Random(f"g2-{cls}-{n}-{seed}")
    if cls == "uniform":
        return [rng.randrange(g.R) for _ in range(n)]
    if cls == "zero":
        return [0] * n
    if cls == "one":
        return [1] * n
    if cls == "rm1":
        return [g.R - 1] * n
    if cls == "bool":                     # fat buckets: nine in ten scalars are 0 or 1
        return [rng.randrange(2) if rng.random() < 0.9 else rng.randrange(g.R) for _ in range(n)]
    raise ValueError(cls)


def pair_classes(col):
    """(duplicate pairs, opposite pairs) of the finite points of the column: lists of index pairs (i, j), i < j"""
    first, dup = {}, []
    for i, q in enumerate(col):
        if q is None:
            continue
        if q in first:
            dup.append((first[q], i))
        else:
            first[q] = i
    opp = []
    for q, i in first.items():
        j = first.get(g.g2_neg(q))
        if j is not None and i < j:
            opp.append((i, j))
    return dup, opp


def pair_scalars(n, pairs, seed):
    """equal scalars on the two members of every pair, zero elsewhere"""
    rng = random.Random(f"g2-pairs-{seed}")
    s = [0] * n
    for i, j in pairs:
        s[i] = s[j] = rng.randrange(1, g.R)
    return s


def fq2_operands():
    """(a, b) lists of Fq2 operands: every pair of the edge elements, then random pairs"""
    rng = random.Random("g2-fq2-kat")
    edge = [(0, 0), (1, 0), (0, 1), (g.P - 1, 0), (g.P - 1, g.P - 1)]
    edge += [(v, _EDGE_FQ[(k + 3) % len(_EDGE_FQ)]) for k, v in enumerate(_EDGE_FQ)]
    a = [x for x in edge for _ in edge] + [(rng.randrange(g.P), rng.randrange(g.P)) for _ in range(64)]
    b = [y for _ in edge for y in edge] + [(rng.randrange(g.P), rng.randrange(g.P)) for _ in range(64)]
    return a, b


FQ2_OPS = {0: "mul", 1: "sqr", 2: "add", 3: "sub", 4: "neg", 5: "mul"}      # uzk_test_g2_kat op -> what it computes


def fq2_expected(op, a, b):
    f = {"mul": g.f2_mul, "add": g.f2_add, "sub": g.f2_sub, "sqr": lambda x, _: g.f2_sqr(x), "neg": lambda x, _: g.f2_neg(x)}[FQ2_OPS[op]]
    return [f(x, y) for x, y in zip(a, b)]


def group_operands(col):
    """(a, b): P + Q, P + P, P + (-P), infinity on either side and on both, for several P, Q of the column"""
    fin = [q for q in col if q is not None]
    a, b = [], []
    for k in range(6):
        p, q = fin[3 * k], fin[3 * k + 1]
        for x, y in ((p, q), (p, p), (p, g.g2_neg(p)), (None, q), (p, None), (None, None), (q, p)):
            a.append(x)
            b.append(y)
    return a, b


def _add(x, y):
    return g.jac_to_affine(g.jac_madd(None if x is None else (x[0], x[1], (1, 0)), y))


GROUP_OPS = (10, 11, 12, 13, 14)


def group_expected(op, a, b):
    out = []
    for x, y in zip(a, b):
        if op in (10, 11):
            r = _add(x, y)
        elif op == 12:
            r = _add(x, x)
        elif op == 13:
            r = _add(x, g.g2_neg(y))
        else:
            s = _add(x, y)
            r = _add(s, s)
        out.append(r)
    return out
