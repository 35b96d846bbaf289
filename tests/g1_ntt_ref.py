"""A G1 NTT composed from the oracle's group operations and its Fr transform (test infrastructure).

Natural order in and out over w = root_of_unity(n):
    forward  out[k] = sum_i w^(ik) in[i]            inverse  out[i] = (1/n) sum_k w^(-ik) in[k]
Points are wire rows [n, 8] (affine, Montgomery coordinates, (0, 0) = infinity), as the product takes and returns them.

  dft_row        row k of the (scaled) DFT matrix, as wire scalars
  g1_ntt_rows    the definition: one MSM per output point (O(n^2): small n)
  g1_ntt         the same by recursive radix-2 splitting with oc.g1_mul / oc.g1_add (O(n log n) scalar multiplications)
  symmetric_ok   the DFT matrix is symmetric, so msm(transform(P), c) == msm(P, transform(c)) for every scalar vector c:
                 one MSM pair checks every output point at once, at any size
"""
import numpy as np

import bn254_py as opy
import oracle_c as oc

G1 = oc.points_from_affine([opy.G1_GEN])[0]
_ONE_Q = oc.fr_from_ints([1], mod=opy.P)[0]
_INF_JAC = np.concatenate([_ONE_Q, _ONE_Q, np.zeros(4, dtype=np.uint64)])


def _to_jac(row):
    if not row.any():
        return _INF_JAC.copy()
    return np.concatenate([row, _ONE_Q])


def dft_row(n, k, inverse=False):
    w = opy.root_of_unity(n)
    if inverse:
        w = pow(w, -1, opy.R)
    wk = pow(w, k, opy.R)
    cur = pow(n, -1, opy.R) if inverse else 1
    row = []
    for _ in range(n):
        row.append(cur)
        cur = cur * wk % opy.R
    return oc.fr_from_ints(row)


def g1_ntt_rows(points, inverse=False):
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    n = p.shape[0]
    return np.stack([oc.g1_to_affine(oc.msm_naive(p, dft_row(n, k, inverse))) for k in range(n)])


def _rec(jacs, w):
    """jacs: list of Jacobian rows, w: a root of unity of order len(jacs) as a canonical int"""
    n = len(jacs)
    if n == 1:
        return jacs
    even, odd = _rec(jacs[0::2], w * w % opy.R), _rec(jacs[1::2], w * w % opy.R)
    out, cur = [None] * n, 1
    for t in range(n // 2):
        o = oc.g1_to_affine(odd[t])
        out[t] = oc.g1_add(even[t], oc.g1_mul(o, oc.fr_from_ints([cur])[0]))
        out[t + n // 2] = oc.g1_add(even[t], oc.g1_mul(o, oc.fr_from_ints([opy.R - cur])[0]))
        cur = cur * w % opy.R
    return out


def g1_ntt(points, inverse=False):
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    n = p.shape[0]
    assert n and n & (n - 1) == 0
    w = opy.root_of_unity(n)
    if inverse:
        w = pow(w, -1, opy.R)
    out = np.stack([oc.g1_to_affine(j) for j in _rec([_to_jac(r) for r in p], w)])
    if inverse:
        ninv = oc.fr_from_ints([pow(n, -1, opy.R)])[0]
        out = np.stack([oc.g1_to_affine(oc.g1_mul(r, ninv)) for r in out])
    return out


def symmetric_ok(points, transformed, c, inverse=False, threads=4):
    """msm(transformed, c) == msm(points, ntt(c)) as affine points"""
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    f = np.ascontiguousarray(transformed, dtype=np.uint64).reshape(-1, 8)
    c = np.ascontiguousarray(c, dtype=np.uint64).reshape(-1, 4)
    lhs = oc.jac_to_affine_ints(oc.msm_pippenger(f, c, 0, threads))
    rhs = oc.jac_to_affine_ints(oc.msm_pippenger(p, oc.ntt(c, inverse=inverse, threads=threads), 0, threads))
    return lhs == rhs


def tau_powers(tau, n):
    """([tau^j] G for j < n as wire rows, the powers as canonical ints)"""
    pw, cur = [], 1
    for _ in range(n):
        pw.append(cur)
        cur = cur * tau % opy.R
    sc = oc.fr_from_ints(pw)
    return np.stack([oc.g1_to_affine(oc.g1_mul(G1, sc[j])) for j in range(n)]), pw
