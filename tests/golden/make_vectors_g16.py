#!/usr/bin/env python3
"""Writes tests/golden/vectors_g16.npz from tests/g16_ref.py and tests/g16_cases.py: for every case of g16_cases.CASES the trapdoor
key, the matrices (CSR), BATCH satisfying assignments with their blinds, h of the first, the proofs, the proofs of the first
assignment with r = s = 0 and r = s = r_mod - 1, and one unsatisfying assignment with its h; for the reference's reveal key
(groth16-reveal-*.bin) over the stand-in system of its shape, the proofs of two assignments.  The GPU tests compare with this file.
About five minutes (the G2 MSMs are Python integers)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import g16_cases as gc     # noqa: E402
import g16_ref as gr       # noqa: E402
import g2_ref as g2        # noqa: E402
import oracle_c as oc      # noqa: E402

KEY_G1 = ("alpha_g1", "beta_g1", "delta_g1")
KEY_G2 = ("beta_g2", "gamma_g2", "delta_g2")
KEY_G1_VEC = ("gamma_abc_g1", "a_query", "b_g1_query", "h_query", "l_query")


def bad_witness(z):
    """one element of a satisfying assignment changed: the last defined output"""
    z = list(z)
    z[-2] = (z[-2] + 1) % gr.R
    return z


def main():
    out = {}
    for name in gc.CASES:
        sy = gc.case_system(name)
        mats = sy.matrices()
        key = gr.trapdoor_setup(mats, sy.l, sy.m, gc.trapdoor(name))
        for f in KEY_G1:
            out[f"{name}_{f}"] = gr.g1_to_wire([getattr(key, f)])[0]
        for f in KEY_G2:
            out[f"{name}_{f}"] = g2.points_to_wire([getattr(key, f)])[0]
        for f in KEY_G1_VEC:
            out[f"{name}_{f}"] = gr.g1_to_wire(getattr(key, f))
        out[f"{name}_b_g2_query"] = g2.points_to_wire(key.b_g2_query)
        for tag, M in zip("ABC", mats):
            out[f"{name}_{tag}_ptr"], out[f"{name}_{tag}_col"], out[f"{name}_{tag}_val"] = gr.csr(M)
        zs = [gc.witness(sy, k) for k in range(gc.BATCH)]
        rs = [gc.blinds(name, k) for k in range(gc.BATCH)]
        assert all(gc.satisfied(sy, z) for z in zs)
        out[f"{name}_z"] = np.stack([oc.fr_from_ints(z) for z in zs])
        out[f"{name}_r"] = oc.fr_from_ints([r for r, _ in rs])
        out[f"{name}_s"] = oc.fr_from_ints([s for _, s in rs])
        hs = [gr.witness_map(mats, sy.l, z) for z in zs]
        assert all(h[-1] == 0 for h in hs)
        out[f"{name}_h"] = oc.fr_from_ints(hs[0])
        out[f"{name}_proofs"] = np.stack([gr.proof_to_wire(gr.prove(key, mats, sy.l, z, r, s, h)) for z, (r, s), h in zip(zs, rs, hs)])
        out[f"{name}_proof_zero"] = gr.proof_to_wire(gr.prove(key, mats, sy.l, zs[0], 0, 0, hs[0]))
        out[f"{name}_proof_rm1"] = gr.proof_to_wire(gr.prove(key, mats, sy.l, zs[0], gr.R - 1, gr.R - 1, hs[0]))
        zb = bad_witness(zs[0])
        assert not gc.satisfied(sy, zb)
        hb = gr.witness_map(mats, sy.l, zb)
        assert hb[-1] != 0
        out[f"{name}_z_bad"], out[f"{name}_h_bad"] = oc.fr_from_ints(zb), oc.fr_from_ints(hb)
        print(name, "done", flush=True)
    sy = gc.real_system()
    key = gr.load_real_key()
    proofs = []
    for k in range(2):
        z = gc.witness(sy, k)
        r, s = gc.blinds("real-shape", k)
        proofs.append(gr.proof_to_wire(gr.prove(key, sy.matrices(), sy.l, z, r, s)))
    out["real_proofs"] = np.stack(proofs)
    path = os.path.join(HERE, "vectors_g16.npz")
    np.savez_compressed(path, **out)
    print("wrote vectors_g16.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
