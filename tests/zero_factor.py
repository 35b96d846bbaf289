"""Inputs of the permutation grand product (helpers.rs:160-220) with ONE chosen factor equal to zero, and the plain restatement that
says what such an input must give (test infrastructure; Python integers throughout, canonical residues mod r).

Row i of the product multiplies z by  prod_j num(j, i) / prod_j den(j, i)  with
    num(j, i) = w[j][i] + gamma + beta * k[j] * group[i]
    den(j, i) = w[j][i] + gamma + beta * k[pv div n] * group[pv mod n],   pv = perm[j][i].
Both are linear in w[j][i], so one wire value makes either of them vanish.  Rows 0 .. n-2 enter the product; row n-1 does not."""
import bn254_py as opy

R = opy.R


def px_of(perm, group, k, i, j):
    n = len(group)
    pv = int(perm[j][i])
    return k[pv // n] * group[pv % n] % R


def zero_numerator(w, perm, group, k, beta, gamma, i, j):
    """Sets w[j][i] so that num(j, i) = 0; returns the value."""
    w[j][i] = -(gamma + beta * k[j] * group[i]) % R
    return w[j][i]


def zero_denominator(w, perm, group, k, beta, gamma, i, j):
    """Sets w[j][i] so that den(j, i) = 0; returns the value.  perm[j][i] must not be the slot (j, i) itself: there numerator and
    denominator are the same factor and would vanish together."""
    n = len(group)
    assert int(perm[j][i]) != j * n + i, "the slot maps to itself: its two factors are one"
    w[j][i] = -(gamma + beta * px_of(perm, group, k, i, j)) % R
    return w[j][i]


def zero_denominator_gamma(w_ji, beta, k, omega, pv, n):
    """The challenge gamma that makes den(j, i) = 0 for the wire value w_ji whose slot maps to pv, over the domain omega^i."""
    return -(w_ji + beta * k[pv // n] * pow(omega, pv % n, R)) % R


def restatement(w, perm, group, k, beta, gamma):
    """helpers.rs:160-220 term by term: (z, nums, dens).  z is None when a denominator of rows 0 .. n-2 is zero (the reference's
    batch_inversion has no inverse to give there)."""
    n, n_wires = len(group), len(w)
    nums, dens = [], []
    for i in range(n - 1):
        nm = dn = 1
        for j in range(n_wires):
            f = w[j][i] + gamma
            nm = nm * ((f + beta * k[j] * group[i]) % R) % R
            dn = dn * ((f + beta * px_of(perm, group, k, i, j)) % R) % R
        nums.append(nm)
        dens.append(dn)
    if any(d == 0 for d in dens):
        return None, nums, dens
    z = [1]
    for nm, dn in zip(nums, dens):
        z.append(z[-1] * nm % R * pow(dn, -1, R) % R)
    return z, nums, dens


class Case:
    """Random inputs of one size, as Python integers (w, group, k, beta, gamma; perm as an array) and in wire format beside them."""

    def __init__(self, n, n_wires=5, seed=1):
        import random

        import numpy as np

        import oracle_c as oc
        rng = random.Random(seed)
        self.n, self.n_wires = n, n_wires
        self.w = [[rng.randrange(R) for _ in range(n)] for _ in range(n_wires)]
        self.group = [rng.randrange(R) for _ in range(n)]
        self.k = [1, 7, 13, 17, 23, 29, 31, 37][:n_wires]
        self.beta, self.gamma = rng.randrange(R), rng.randrange(R)
        self.perm = np.random.default_rng(seed).integers(0, n * n_wires, size=(n_wires, n), dtype=np.uint32)
        self.w_wire = oc.fr_from_ints([v for row in self.w for v in row]).reshape(n_wires, n, 4)
        self.group_wire, self.k_wire = oc.fr_from_ints(self.group), oc.fr_from_ints(self.k)
        self.beta_wire, self.gamma_wire = oc.fr_from_ints([self.beta, self.gamma])

    def ints(self):
        return self.w, self.perm, self.group, self.k, self.beta, self.gamma

    def wires(self, w_wire=None):
        return (self.w_wire if w_wire is None else w_wire), self.perm, self.group_wire, self.k_wire, self.beta_wire, self.gamma_wire

    def free_wire(self, i, avoid=()):
        """A wire j of row i whose slot does not map to itself (zero_denominator's condition) and is not in `avoid`."""
        return next(j for j in range(self.n_wires) if j not in avoid and int(self.perm[j][i]) != j * self.n + i)

    def with_zeros(self, zeros):
        """zeros: (kind, row, wire) with kind "num" | "den".  Returns the wire-format witness with those factors zero; the integer
        witness of the case is left as it was."""
        import oracle_c as oc
        out = self.w_wire.copy()
        for kind, i, j in zeros:
            keep = self.w[j][i]
            v = (zero_numerator if kind == "num" else zero_denominator)(*self.ints(), i, j)
            self.w[j][i] = keep
            out[j, i] = oc.fr_from_ints([v])[0]
        return out
