"""The SRS check restated with the oracle (test infrastructure, no tests): the fold weights through the golden verifier's
Keccak-256, the curve report through the Python integers of bn254_py, the fold through the C oracle's Pippenger, the verdict
through the oracle pairing.  Points are wire rows [n, 8] (Montgomery coordinates, (0, 0) = infinity), as the product takes them."""
import numpy as np

import bn254_pairing as pr
import bn254_py as opy
import oracle_c as oc
from g1_ntt_ref import tau_powers  # noqa: F401  (re-exported: ([tau^j] G as wire rows, the powers))
from plonk_golden_verifier import keccak256

DOMAIN = b"uzksrsv1"


def weights_ints(seed, first, count):
    """rho_first .. rho_(first + count - 1): block j = keccak256(seed || "uzksrsv1" || le64(j)), bytes 0..15 and 16..31 little endian"""
    assert len(seed) == 32
    out = []
    for k in range(first, first + count):
        d = keccak256(bytes(seed) + DOMAIN + (k // 2).to_bytes(8, "little"))
        out.append(int.from_bytes(d[16 * (k % 2):16 * (k % 2) + 16], "little"))
    return out


def weights_wire(seed, first, count):
    return oc.fr_from_ints(weights_ints(seed, first, count)) if count else np.zeros((0, 4), dtype=np.uint64)


def _raw(row, k):
    return sum(int(row[4 * k + j]) << (64 * j) for j in range(4))


def classify(row):
    """'infinity' | 'non_canonical' | 'off_curve' | 'good' of one wire row"""
    x, y = _raw(row, 0), _raw(row, 1)
    if x == 0 and y == 0:
        return "infinity"
    if x >= opy.P or y >= opy.P:
        return "non_canonical"
    return "good" if opy.g1_is_on_curve((opy.from_mont(x, opy.P), opy.from_mont(y, opy.P))) else "off_curve"


def curve_report(wire, offset=0, count=None):
    wire = np.ascontiguousarray(wire, dtype=np.uint64).reshape(-1, 8)
    count = wire.shape[0] - offset if count is None else count
    rep = {"checked": count, "infinity": 0, "non_canonical": 0, "off_curve": 0, "first_bad": None}
    for i in range(offset, offset + count):
        c = classify(wire[i])
        if c != "good":
            rep[c] += 1
        if c in ("non_canonical", "off_curve") and rep["first_bad"] is None:
            rep["first_bad"] = i
    return rep


def fold(wire, seed, offset=0, count=None, threads=4):
    """(left, right) as affine wire rows [8]: the oracle's two MSMs over the run under the weights of the seed"""
    wire = np.ascontiguousarray(wire, dtype=np.uint64).reshape(-1, 8)
    count = wire.shape[0] - offset if count is None else count
    w = weights_wire(seed, 0, count - 1)
    left = oc.msm_pippenger(wire[offset:offset + count - 1], w, 0, threads)
    right = oc.msm_pippenger(wire[offset + 1:offset + count], w, 0, threads)
    return oc.g1_to_affine(left), oc.g1_to_affine(right)


def affine_wire(jac):
    """a Jacobian result [12] of the product as an affine wire row [8]"""
    return oc.g1_to_affine(np.ascontiguousarray(jac, dtype=np.uint64))


def pairing_accepts(left, right, g2):
    """e(right, H) == e(left, [tau] H) with g2 = (H, [tau] H); left, right Jacobian [12] of the product"""
    l, r = oc.jac_to_affine_ints(left), oc.jac_to_affine_ints(right)
    return pr.pairing_product_is_one([(r, g2[0]), (opy.g1_neg(l), g2[1])])
