"""CPU restatement, on Python integers, of the DEVICE's pairing (uzkge_amd/csrc/fq12_29.hpp, pairing.hip) -- the algorithm, not the
limbs: Fq12 as six Fq2 coefficients of w (w^6 = xi = 9 + u), every product computed one OUTPUT coefficient at a time as a lane of the
kernel does (the second operand is read from a table of twelve entries, b_j and xi b_j, so that a wrapped index costs no branch), the
product by a sparse line (coefficients at w^0, w^1, w^3), the Granger-Scott square of the cyclotomic subgroup, Frobenius maps by
constants xi^(k (p^j - 1) / 6), the inverse by the norm chain (f conj(f) lies in Fq6, its norm to Fq2 is t t^(p^2) t^(p^4): ONE Fq
inversion), the Miller loop with T in homogeneous projective coordinates (no inversion; every line differs from the oracle's affine
one by a factor in Fq2, which the final exponentiation removes) and the final exponentiation with the hard part (p^4 - p^2 + 1) / r
computed EXACTLY from its base-p expansion.  tests/test_pairing_ref_host.py holds all of it to oracle/bn254_pairing.py."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import bn254_pairing as op  # noqa: E402
from bn254_pairing import BN_X, P, R, XI, f2_add, f2_conj, f2_inv, f2_mul, f2_neg, f2_pow, f2_scale, f2_sqr, f2_sub  # noqa: E402

ZERO2, ONE2 = (0, 0), (1, 0)
F12_ONE = [ONE2] + [ZERO2] * 5
ATE_LOOP = 6 * BN_X + 2                     # 65 bits
TWIST_B = op.TWIST_B

# gamma[j][k] = xi^(k (p^j - 1) / 6), j = 1, 2, 3, from g = xi^((p - 1) / 6) alone (what the host does at start-up):
# gamma[1][k] = g^k, gamma[2][k] = gamma[1][k] conj(gamma[1][k]), gamma[3][k] = gamma[1][k] gamma[2][k]
_G = f2_pow(XI, (P - 1) // 6)
GAMMA = {1: [f2_pow(_G, k) for k in range(6)]}
GAMMA[2] = [f2_mul(g, f2_conj(g)) for g in GAMMA[1]]
GAMMA[3] = [f2_mul(a, b) for a, b in zip(GAMMA[1], GAMMA[2])]


def xi_mul(a):
    return ((9 * a[0] - a[1]) % P, (a[0] + 9 * a[1]) % P)


def table(b):
    """b_0 .. b_5, then xi b_0 .. xi b_5: the second operand of a product as the lanes read it"""
    return list(b) + [xi_mul(c) for c in b]


def mul_coeff(a, tb, k):
    """coefficient k of a b: sum_i a_i b'_(k - i), the wrapped ones (i > k) through the xi half of the table"""
    acc = ZERO2
    for i in range(6):
        j = k - i
        acc = f2_add(acc, f2_mul(a[i], tb[j] if j >= 0 else tb[j + 12]))
    return acc


def f12_mul(a, b):
    tb = table(b)
    return [mul_coeff(a, tb, k) for k in range(6)]


def f12_sqr(a):
    return f12_mul(a, a)


def sparse_coeff(a, ell, k):
    """coefficient k of a (l0 + l1 w + l3 w^3)"""
    l0, l1, l3 = ell
    t1 = l1 if k >= 1 else xi_mul(l1)
    t3 = l3 if k >= 3 else xi_mul(l3)
    return f2_add(f2_add(f2_mul(a[k], l0), f2_mul(a[(k + 5) % 6], t1)), f2_mul(a[(k + 3) % 6], t3))


def f12_mul_sparse(a, ell):
    return [sparse_coeff(a, ell, k) for k in range(6)]


def f12_conj(a):
    """the p^6 map: w -> -w"""
    return [c if k % 2 == 0 else f2_neg(c) for k, c in enumerate(a)]


def f12_frob(a, j):
    return [f2_mul(f2_conj(c) if j & 1 else c, GAMMA[j][k]) for k, c in enumerate(a)]


# Granger-Scott: with a = sum a_k w^k in the cyclotomic subgroup, the three Fq4 pairs are (a0, a3), (a1, a4), (a2, a5)
CYC_X = (0, 2, 1, 0, 2, 1)                  # lane k squares the pair (a_x, a_(x + 3)), x = CYC_X[k]


def cyc_coeff(a, k):
    x, y = a[CYC_X[k]], a[CYC_X[k] + 3]
    if k % 2 == 0:                          # 3 (x^2 + xi y^2) - 2 a_k
        t = f2_add(f2_mul(x, x), f2_mul(xi_mul(y), y))
        return f2_sub(f2_scale(t, 3), f2_scale(a[k], 2))
    t = f2_mul(x, xi_mul(y) if k == 1 else y)    # 3 (2 x y) + 2 a_k, with xi for the pair that wraps
    return f2_add(f2_scale(t, 6), f2_scale(a[k], 2))


def f12_cyc_sqr(a):
    return [cyc_coeff(a, k) for k in range(6)]


def fq_inv(a):
    return pow(a, P - 2, P)                 # 0 -> 0


def f12_inv(a):
    """a^-1 = conj(a) t' t'' / N, t = a conj(a) (in Fq6: odd coefficients zero), t' = t^(p^2), t'' = t^(p^4), N = t t' t'' in Fq2.
    The inverse of 0 is 0."""
    c = f12_conj(a)
    t = f12_mul(a, c)
    t1 = f12_frob(t, 2)
    t2 = f12_frob(t1, 2)
    m = f12_mul(t1, t2)
    n = mul_coeff(t, table(m), 0)
    d = fq_inv((n[0] * n[0] + n[1] * n[1]) % P)
    ninv = (n[0] * d % P, (-n[1]) * d % P)
    return [f2_mul(x, ninv) for x in f12_mul(c, m)]


# ---- Miller loop ------------------------------------------------------------------------------------
def dbl_step(t):
    """T = 2 T in homogeneous projective coordinates on the twist (Costello-Lange-Naehrig's doubling with every coordinate times 4, so
    that no halving is needed), and the tangent's coefficients (the one at w^0 still to be multiplied by -yP, at w^1 by xP, w^3)"""
    x, y, z = t
    b = f2_sqr(y)
    c = f2_sqr(z)
    e = f2_mul(c, f2_scale(TWIST_B, 3))
    f = f2_scale(e, 3)
    h = f2_sub(f2_sqr(f2_add(y, z)), f2_add(b, c))               # 2 y z
    i = f2_sub(e, b)
    j = f2_sqr(x)
    xy = f2_mul(x, y)
    t3 = (f2_mul(f2_add(xy, xy), f2_sub(b, f)), f2_sub(f2_sqr(f2_add(b, f)), f2_scale(f2_sqr(f2_add(e, e)), 3)), f2_scale(f2_mul(b, h), 4))
    return t3, (h, f2_scale(j, 3), i)


def add_step(t, q):
    """T = T + Q (Q affine) and the chord's coefficients, the whole line negated (same convention: -yP, xP, 1)"""
    x, y, z = t
    theta = f2_sub(y, f2_mul(q[1], z))
    lam = f2_sub(x, f2_mul(q[0], z))
    c = f2_sqr(theta)
    d = f2_sqr(lam)
    e = f2_mul(lam, d)
    f = f2_mul(z, c)
    g = f2_mul(x, d)
    h = f2_sub(f2_add(e, f), f2_scale(g, 2))
    t3 = (f2_mul(lam, h), f2_sub(f2_mul(theta, f2_sub(g, h)), f2_mul(e, y)), f2_mul(z, e))
    j = f2_sub(f2_mul(lam, q[1]), f2_mul(theta, q[0]))
    return t3, (lam, theta, j)


def line_at(co, p):
    return (f2_scale(co[0], P - p[1]), f2_scale(co[1], p[0]), co[2])


def miller_loop(p, q):
    if p is None or q is None:
        return list(F12_ONE)
    f = list(F12_ONE)
    t = (q[0], q[1], ONE2)
    for bit in bin(ATE_LOOP)[3:]:
        t, co = dbl_step(t)
        f = f12_mul_sparse(f12_sqr(f), line_at(co, p))
        if bit == "1":
            t, co = add_step(t, q)
            f = f12_mul_sparse(f, line_at(co, p))
    q1 = (f2_mul(f2_conj(q[0]), GAMMA[1][2]), f2_mul(f2_conj(q[1]), GAMMA[1][3]))
    q2 = (f2_mul(q[0], GAMMA[2][2]), f2_neg(f2_mul(q[1], GAMMA[2][3])))
    t, co = add_step(t, q1)
    f = f12_mul_sparse(f, line_at(co, p))
    t, co = add_step(t, q2)
    return f12_mul_sparse(f, line_at(co, p))


# ---- final exponentiation ---------------------------------------------------------------------------
def easy_part(f):
    g = f12_mul(f12_conj(f), f12_inv(f))    # f^(p^6 - 1)
    return f12_mul(f12_frob(g, 2), g)       # ^(p^2 + 1)


def cyc_pow_x(a):
    r = a
    for bit in bin(BN_X)[3:]:
        r = f12_cyc_sqr(r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def _pow6(a):
    return f12_cyc_sqr(f12_mul(f12_cyc_sqr(a), a))


HARD = (P ** 4 - P ** 2 + 1) // R
L0, L1, L2 = -36 * BN_X ** 3 - 30 * BN_X ** 2 - 18 * BN_X - 2, -36 * BN_X ** 3 - 18 * BN_X ** 2 - 12 * BN_X + 1, 6 * BN_X ** 2 + 1
assert HARD == P ** 3 + L2 * P ** 2 + L1 * P + L0 and (P ** 12 - 1) // R == (P ** 6 - 1) * (P ** 2 + 1) * HARD


def hard_part(f):
    """f^((p^4 - p^2 + 1) / r) exactly: f^L0 (f^L1)^p (f^L2)^(p^2) f^(p^3); inversion is conjugation in the cyclotomic subgroup"""
    fx = cyc_pow_x(f)
    fx2 = cyc_pow_x(fx)
    fx3 = cyc_pow_x(fx2)
    a, b, c36 = _pow6(fx), _pow6(fx2), _pow6(_pow6(fx3))
    a2, b2 = f12_cyc_sqr(a), f12_cyc_sqr(b)
    b3 = f12_mul(b2, b)
    t = f12_mul(f12_mul(c36, b3), a2)                   # f^(36 x^3 + 18 x^2 + 12 x)
    y1 = f12_mul(f12_conj(t), f)                        # f^L1
    y0 = f12_conj(f12_mul(f12_mul(f12_mul(t, b2), a), f12_cyc_sqr(f)))   # f^L0
    y2 = f12_mul(b, f)                                  # f^L2
    r = f12_mul(y0, f12_frob(y1, 1))
    r = f12_mul(r, f12_frob(y2, 2))
    return f12_mul(r, f12_frob(f, 3))


def final_exponentiation(f):
    return hard_part(easy_part(f))


def pairing_product(pairs):
    f = list(F12_ONE)
    for p, q in pairs:
        f = f12_mul(f, miller_loop(p, q))
    return final_exponentiation(f)
