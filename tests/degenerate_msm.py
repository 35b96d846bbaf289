"""Degenerate base sets for the MSM tests, with a closed-form expected result (test infrastructure).

Every base is k * G with a KNOWN discrete log k (k = 0: infinity, wire zeros), so the expected MSM result needs no second
Pippenger: it is (sum_i s_i * k_i mod r) * G by Python integers and one opy.g1_mul, or None (infinity) when the sum is 0.
The bases repeat, come in opposite pairs, or are powers of two of one point -- the inputs on which the group additions inside
the MSM kernels degenerate (doubling, cancellation), which distinct SRS points never do.

  pool(family)                      (discrete logs, wire rows [m, 8]) of a family's distinct points, built once (m <= 254)
  bases(family, n, period)          (index into the pool [n], wire rows [n, 8])
  scalars(kind, n, period)          (canonical ints, wire rows [n, 4])
  case(family, kind, n, ...)        a Case: points, scalars, and the closed-form result `want` -- cached, shared, read-only

Base families
  one_point    every base is the same k * G
  plus_minus   k * G and -k * G: the sign alternates by index, or (period = p) changes every p bases, so whole chunks cancel
  pool64       30 random logs, their 30 negatives and 4 infinities, indexed uniformly: sparse degeneracy
  pow2         logs 2^u, u < 254, indexed uniformly: what a monomial SRS looks like when tau is a power of two
Scalar kinds
  uniform      n uniform values
  pow2         +-2^t: one non-zero digit each (negative digits through r - 2^t)
  periodic     `period` uniform values, repeated
  same         one value n times: one bucket per window
  cancel       the second half is the negation of the first (an odd n ends with a zero)
"""
import functools
import random
from collections import namedtuple

import numpy as np

import bn254_py as opy
import oracle_c as oc

FAMILIES = ("one_point", "plus_minus", "pool64", "pow2")
KINDS = ("uniform", "pow2", "periodic", "same", "cancel")

_K = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % opy.R     # the log of one_point / plus_minus

Case = namedtuple("Case", "points scalars want idx ints logs")


@functools.lru_cache(maxsize=None)
def pool(family):
    if family == "one_point":
        logs = [_K]
    elif family == "plus_minus":
        logs = [_K, opy.R - _K]
    elif family == "pool64":
        rng = random.Random(6464)
        pos = [rng.randrange(1, opy.R) for _ in range(30)]
        logs = pos + [opy.R - k for k in pos] + [0] * 4
    elif family == "pow2":
        logs = [1 << u for u in range(254)]
    else:
        raise ValueError(family)
    assert len(logs) <= 254
    wire = oc.points_from_affine([opy.g1_mul(opy.G1_GEN, k) for k in logs])
    wire.setflags(write=False)
    return logs, wire


def bases(family, n, period=None, seed=0):
    logs, wire = pool(family)
    if family == "one_point":
        idx = np.zeros(n, dtype=np.int64)
    elif family == "plus_minus":
        idx = (np.arange(n, dtype=np.int64) // (period or 1)) & 1
    else:
        idx = np.random.default_rng(1000 + seed).integers(0, len(logs), n)
    return idx, wire[idx]


def scalars(kind, n, period=None, seed=0):
    rng = random.Random(f"{kind}/{n}/{period}/{seed}")
    if kind == "uniform":
        vals = [rng.randrange(opy.R) for _ in range(n)]
        sel = np.arange(n)
    elif kind == "pow2":
        vals = [1 << t for t in range(254)] + [opy.R - (1 << t) for t in range(254)]
        sel = np.random.default_rng(2000 + seed).integers(0, len(vals), n)
    elif kind == "periodic":
        vals = [rng.randrange(opy.R) for _ in range(period)]
        sel = np.arange(n) % period
    elif kind == "same":
        vals = [rng.randrange(1, opy.R)]
        sel = np.zeros(n, dtype=np.int64)
    elif kind == "cancel":
        h = n // 2
        first = [rng.randrange(opy.R) for _ in range(h)]
        vals = first + [(opy.R - v) % opy.R for v in first] + [0]
        sel = np.concatenate([np.arange(2 * h), np.full(n - 2 * h, 2 * h)]).astype(np.int64)
    else:
        raise ValueError(kind)
    ints = [vals[j] for j in sel.tolist()]
    return ints, oc.fr_from_ints(vals)[sel]


def closed_form(logs, idx, ints):
    """(sum_i s_i * k_i mod r) * G as a canonical affine point, None for infinity"""
    total = sum(s * logs[j] for s, j in zip(ints, idx.tolist())) % opy.R
    return opy.g1_mul(opy.G1_GEN, total) if total else None


def default_period(n):
    """the period of `periodic` scalars where a test names none: at least four repeats"""
    return max(1, min(1024, n // 4))


@functools.lru_cache(maxsize=24)
def case(family, kind, n, base_period=None, scalar_period=None, seed=0):
    if kind == "periodic" and scalar_period is None:
        scalar_period = default_period(n)
    logs, _ = pool(family)
    idx, pts = bases(family, n, base_period, seed)
    ints, sc = scalars(kind, n, scalar_period, seed)
    pts.setflags(write=False)
    sc.setflags(write=False)
    return Case(pts, sc, closed_form(logs, idx, ints), idx, ints, logs)
