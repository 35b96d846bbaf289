#!/usr/bin/env python3
"""Writes tests/golden/vectors_g2.npz from tests/g2_ref.py (Python integers): the expected affine outputs of the G2 MSM cases of
tests/g2_cases.py over the b_g2_query column of groth16-reveal-b-queries.bin, and the operands and results of the Fq2 / G2
known-answer cases.  The GPU tests compare with this file and never run the Python Pippenger.  About two minutes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import g2_cases as gc      # noqa: E402
import g2_ref as g         # noqa: E402


def main():
    _, col = g.load_fixture()
    out = {}
    for n in gc.SIZES:
        for cls in gc.CLASSES:
            out[f"msm_{cls}_{n}"] = g.points_to_wire([g.msm(col[:n], gc.scalars(cls, n))])[0]
    dup, opp = gc.pair_classes(col)
    assert (len(dup), len(opp)) == (256, 254)
    out["msm_dup_pairs"] = g.points_to_wire([g.msm(col, gc.pair_scalars(len(col), dup, 1))])[0]
    out["msm_opp_pairs"] = g.points_to_wire([g.msm(col, gc.pair_scalars(len(col), opp, 2))])[0]
    assert not out["msm_opp_pairs"].any()
    off, n = gc.OFFSET_CASE
    out["msm_offset"] = g.points_to_wire([g.msm(col[off:off + n], gc.scalars("uniform", n, seed=3))])[0]
    for b in range(8):
        out[f"msm_batch_{b}"] = g.points_to_wire([g.msm(col, gc.scalars("uniform", len(col), seed=10 + b))])[0]
    a, b = gc.fq2_operands()
    out["fq2_a"] = np.stack([g.fq2_to_wire(x) for x in a])
    out["fq2_b"] = np.stack([g.fq2_to_wire(x) for x in b])
    for op in gc.FQ2_OPS:
        out[f"fq2_op{op}"] = np.stack([g.fq2_to_wire(x) for x in gc.fq2_expected(op, a, b)])
    a, b = gc.group_operands(col)
    out["grp_a"], out["grp_b"] = g.points_to_wire(a), g.points_to_wire(b)
    for op in gc.GROUP_OPS:
        out[f"grp_op{op}"] = g.points_to_wire(gc.group_expected(op, a, b))
    np.savez_compressed(os.path.join(HERE, "vectors_g2.npz"), **out)
    print("wrote vectors_g2.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
