"""A Groth16 proving key of ANY size whose every point has a known discrete logarithm, for proofs with a closed form at domains where
g16_ref.trapdoor_setup (one Python scalar multiplication per key point) is out of reach.

Every query point is c G (or c G2) with c taken from a small fixed POOL of scalars: the pool's points are computed once (O(pool) curve
operations), and a column of any length is the pool's wire table indexed by a seeded draw -- numpy does the rest.  The five columns
(a_query, b_g1_query, b_g2_query, l_query, h_query) are drawn independently, so b_g1_query and b_g2_query carry DIFFERENT logarithms
and a prover that mixed them up would show; alpha, beta (in G1 and in G2) and delta (in G1 and in G2) are independent known scalars
too.  Such a key is no one's trusted setup and its proofs do not verify; what it gives is the value of every MSM as Python integers:

    a  = alpha + sum z_i ca_i + r delta_1          b1 = beta_1 + sum z_i cb1_i + s delta_1       b2 = beta_2 + sum z_i cb2_i + s delta_2
    k  = sum z_{l+i} cl_i + sum h_i ch_i - r s delta_1                                            c  = s a + r b1 + k
    proof = (a G, b2 G2, c G)                                                                     (g16_ref.closed_form_logs)

The pool holds 0 (the point at infinity), 1, r - 1, a scalar k with r - k (an opposite pair) and 2 k, and random others.  Every column
long enough gets the infinity, the opposite pair, k a second time (a duplicate) and 2 k at seeded positions, whatever else the draw
brings; `drawn` reports what a column holds."""
import random

import numpy as np

import g16_ref as gr
import g2_ref as g2

R = gr.R
POOL_G1 = 64
POOL_G2 = 128                  # 5 ms per G2 point through g16_ref._g2_fixed: the table is built in under a second
COLUMNS = ("a", "b1", "b2", "l", "h")
_SPECIAL = (0, 3, 4, 3, 5)     # pool indices forced into every column of >= 5 points: infinity, k, r - k, k again, 2 k

_tables = {}


def pool(group):
    """the pool's scalars: [0, 1, r - 1, k, r - k, 2 k, random ...]; group is "g1" or "g2" (independent pools)"""
    rng = random.Random(f"g16-pool-{group}")
    k = rng.randrange(2, R // 2)
    size = POOL_G1 if group == "g1" else POOL_G2
    return [0, 1, R - 1, k, R - k, 2 * k % R] + [rng.randrange(2, R - 1) for _ in range(size - 6)]


def table(group):
    """(scalars, wire rows [pool, 8] or [pool, 16]) of the pool's points"""
    if group not in _tables:
        sc = pool(group)
        if group == "g1":
            mul = gr._g1_fixed()
            _tables[group] = (sc, gr.g1_to_wire([mul(c) for c in sc]))
        else:
            mul = gr._g2_fixed()
            _tables[group] = (sc, g2.points_to_wire([mul(c) for c in sc]))
    return _tables[group]


def _draw(name, column, length, size):
    """pool indices of one column: a seeded uniform draw, the special entries written over seeded distinct positions"""
    seed = int.from_bytes(f"g16-pool-{name}-{column}".encode(), "little") % (1 << 63)
    idx = np.random.default_rng(seed).integers(0, size, size=length, dtype=np.int64)
    if length >= len(_SPECIAL):
        at = random.Random(f"g16-pool-at-{name}-{column}").sample(range(length), len(_SPECIAL))
        idx[at] = _SPECIAL
    return idx


class PoolKey:
    """logs: the dictionary g16_ref.closed_form_logs takes (lists of Python integers); arrays: the keyword arguments of
    backend.Groth16Key.from_arrays apart from the matrices; idx: column -> pool indices"""

    def __init__(self, name, m, l, n):
        rng = random.Random(f"g16-pool-fixed-{name}")
        s1, t1 = table("g1")
        s2, t2 = table("g2")
        lens = {"a": m, "b1": m, "b2": m, "l": m - l, "h": n - 1}
        self.name, self.m, self.l, self.n = name, m, l, n
        self.idx = {c: _draw(name, c, lens[c], len(s2 if c == "b2" else s1)) for c in COLUMNS}
        self.logs = {c: [(s2 if c == "b2" else s1)[i] for i in self.idx[c]] for c in COLUMNS}
        fixed = {f: rng.randrange(1, R) for f in ("alpha", "beta_g1", "beta_g2", "delta_g1", "delta_g2")}
        self.logs.update(fixed)
        m1, m2 = gr._g1_fixed(), gr._g2_fixed()
        col = lambda c: (t2 if c == "b2" else t1)[self.idx[c]]
        self.arrays = dict(alpha_g1=gr.g1_to_wire([m1(fixed["alpha"])])[0], beta_g1=gr.g1_to_wire([m1(fixed["beta_g1"])])[0],
                           delta_g1=gr.g1_to_wire([m1(fixed["delta_g1"])])[0], beta_g2=g2.points_to_wire([m2(fixed["beta_g2"])])[0],
                           delta_g2=g2.points_to_wire([m2(fixed["delta_g2"])])[0], a_query=col("a"), b_g1_query=col("b1"), l_query=col("l"),
                           h_query=col("h"), b_g2_query=col("b2"))

    def drawn(self, column):
        """what the column holds: (infinities, opposite pairs among its distinct scalars, entries that repeat an earlier one)"""
        logs = self.logs[column]
        seen = set(logs)
        pairs = sum(1 for c in seen if c and c < R - c and R - c in seen)
        return logs.count(0), pairs, len(logs) - len(seen)

    def ref_key(self):
        """the same key as g16_ref.Key (points as integer tuples): what g16_ref.prove takes.  O(size) Python; small keys only."""
        s1, t1 = table("g1")
        s2, t2 = table("g2")
        p1, p2 = gr.g1_from_wire(t1), [g2.point_from_wire(w) for w in t2]
        g1col = lambda c: [p1[i] for i in self.idx[c]]
        a = self.arrays
        return gr.Key(alpha_g1=gr.g1_from_wire(a["alpha_g1"])[0], beta_g1=gr.g1_from_wire(a["beta_g1"])[0], delta_g1=gr.g1_from_wire(a["delta_g1"])[0],
                      beta_g2=g2.point_from_wire(a["beta_g2"]), gamma_g2=None, delta_g2=g2.point_from_wire(a["delta_g2"]), gamma_abc_g1=[],
                      a_query=g1col("a"), b_g1_query=g1col("b1"), b_g2_query=[p2[i] for i in self.idx["b2"]], h_query=g1col("h"), l_query=g1col("l"))

    def from_arrays_args(self, sy):
        """the keyword arguments of backend.Groth16Key.from_arrays for this key over the system's matrices"""
        assert (sy.m, sy.l, sy.n) == (self.m, self.l, self.n)
        return dict(n_vars=sy.m, n_inputs=sy.l, n_constraints=sy.nc, matrices=[gr.csr(M) for M in sy.matrices()], **self.arrays)
