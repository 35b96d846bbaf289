"""CPU restatement of the Groth16 prover of include/uzkge_gpu.h (uzk_g16_*): Python integers for the protocol, the C oracle for the
transforms and the G1 MSMs, tests/g2_ref.py for G2.

  parse_key         ark-serialize (compressed) ProvingKey<Bn254>, as the reference's shuffle/parameters/groth16_pk.bin
  witness_map       ark-groth16's LibsnarkReduction::witness_map_from_matrices as the header states it
  prove             A, B, C of a proof from a key, the matrices, an assignment and the blinds r, s
  trapdoor_setup    a key for a given R1CS from known tau, alpha, beta, gamma, delta: every query point is a known scalar times the
                    generator, so a proof has a closed form (closed_form) and can be verified (verify)
  closed_form_logs  that closed form for ANY key whose points' logarithms are known (a trapdoor key, or tests/g16_pool.py's)

G1 points are affine integer tuples (x, y), G2 points ((x0, x1), (y0, y1)); None = infinity.  Rows of a matrix are lists of
(column, value)."""
import hashlib
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import bn254_pairing as pr      # noqa: E402
import bn254_py as opy          # noqa: E402
import g2_ref as g2             # noqa: E402
import oracle_c as oc           # noqa: E402

R, P = opy.R, opy.P
GEN = 5                                          # Fr::GENERATOR: the coset shift
GOLDEN = os.path.join(HERE, "golden")
HEAD = os.path.join(GOLDEN, "groth16-reveal-head.bin")        # bytes [0, 156336) of groth16_pk.bin
TAIL = os.path.join(GOLDEN, "groth16-reveal-tail.bin")        # bytes [623776, 1041488)
HEAD_SHA256 = "ab8ffe014616a23935fbc34b230894116b1febf2e374296dc1175fe6454bf22c"
TAIL_SHA256 = "4832d4756108001550af3b59a6efafc1e5b633d1aa3a0a786d7ed130f8113a83"
SECTION_LENS = (7, 4869, 4869, 4869, 8191, 4862)              # gamma_abc_g1, a_query, b_g1_query, b_g2_query, h_query, l_query


class Key:
    """alpha_g1, beta_g1, delta_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1[l], a_query[m], b_g1_query[m], b_g2_query[m],
    h_query[n - 1], l_query[m - l]"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---- the key file -----------------------------------------------------------------------------------------------------------
def parse_key(data, g1=g2.decompress_g1, g2_=g2.decompress_g2):
    """ark-serialize, compressed: vk = alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | Vec gamma_abc_g1, then beta_g1 | delta_g1 | Vec
    a_query | Vec b_g1_query | Vec b_g2_query | Vec h_query | Vec l_query; a Vec is u64 LE length then the elements (G1 32 B, G2 64 B)"""
    pos = [0]

    def p1():
        pos[0] += 32
        return g1(data[pos[0] - 32:pos[0]])

    def p2():
        pos[0] += 64
        return g2_(data[pos[0] - 64:pos[0]])

    def vec(f):
        n = struct.unpack_from("<Q", data, pos[0])[0]
        pos[0] += 8
        return [f() for _ in range(n)]

    k = Key()
    k.alpha_g1, k.beta_g2, k.gamma_g2, k.delta_g2 = p1(), p2(), p2(), p2()
    k.gamma_abc_g1 = vec(p1)
    k.beta_g1, k.delta_g1 = p1(), p1()
    k.a_query, k.b_g1_query, k.b_g2_query, k.h_query, k.l_query = vec(p1), vec(p1), vec(p2), vec(p1), vec(p1)
    assert pos[0] == len(data)
    return k


_cache = {}


def load_real_key():
    """the reference's reveal key from the three fixtures (head | b-queries | tail)"""
    if "key" not in _cache:
        data = open(HEAD, "rb").read() + open(g2.FIXTURE, "rb").read() + open(TAIL, "rb").read()
        _cache["key"] = parse_key(data)
    return _cache["key"]


# ---- the witness map ----------------------------------------------------------------------------------------------------------
def domain_of(nc, l):
    n = 1
    while n < nc + l:
        n <<= 1
    return n


def _dot(row, z):
    return sum(v * z[c] for c, v in row) % R


def _scale_pows(v, k):
    out, p = [], 1
    for x in v:
        out.append(x * p % R)
        p = p * k % R
    return out


def _ntt(v, inverse=False):
    return oc.fr_to_ints(oc.ntt(oc.fr_from_ints(v), inverse=inverse))


def witness_map(matrices, l, z):
    """h: n coefficients"""
    A, B, C = matrices
    nc = len(A)
    n = domain_of(nc, l)
    a = [_dot(r, z) for r in A] + [z[j] for j in range(l)] + [0] * (n - nc - l)
    b = [_dot(r, z) for r in B] + [0] * (n - nc)
    c = [_dot(r, z) for r in C] + [0] * (n - nc)
    a, b, c = (_ntt(_scale_pows(_ntt(v, inverse=True), GEN)) for v in (a, b, c))
    zi = pow(pow(GEN, n, R) - 1, R - 2, R)
    t = [(x * y - w) * zi % R for x, y, w in zip(a, b, c)]
    return _scale_pows(_ntt(t, inverse=True), pow(GEN, R - 2, R))


# ---- the prover ---------------------------------------------------------------------------------------------------------------
def _msm_g1(points, scalars):
    pts = oc.points_from_affine([p if p is not None else (0, 0) for p in points])
    return oc.jac_to_affine_ints(oc.msm_pippenger(pts, oc.fr_from_ints(scalars)))


def _g1(p):
    return None if p in (None, (0, 0)) else p


def prove(key, matrices, l, z, r, s, h=None):
    """(A, B, C) affine; h may be passed when it is known already"""
    h = witness_map(matrices, l, z) if h is None else h
    n = len(h)
    A = _g1(_msm_g1(key.a_query + [key.alpha_g1, key.delta_g1], z + [1, r]))
    B1 = _g1(_msm_g1(key.b_g1_query + [key.beta_g1, key.delta_g1], z + [1, s]))
    B = g2.msm(key.b_g2_query + [key.beta_g2, key.delta_g2], z + [1, s])
    K = _g1(_msm_g1(key.l_query + key.h_query + [key.delta_g1], z[l:] + h[:n - 1] + [(-r * s) % R]))
    C = opy.g1_add(opy.g1_add(opy.g1_mul(A, s), opy.g1_mul(B1, r)), K)
    return A, B, _g1(C)


# ---- trapdoor setup -----------------------------------------------------------------------------------------------------------
def lagrange_at(n, tau):
    """L_i(tau) over the size-n domain, i < n"""
    w = opy.root_of_unity(n)
    zt = (pow(tau, n, R) - 1) * pow(n, R - 2, R) % R
    out, wi = [], 1
    for _ in range(n):
        out.append(zt * wi % R * pow((tau - wi) % R, R - 2, R) % R)
        wi = wi * w % R
    return out


def qap_at(matrices, l, m, tau):
    """u_j(tau), v_j(tau), w_j(tau) for j < m; A carries the l input-consistency rows behind its constraints"""
    A, B, C = matrices
    nc = len(A)
    L = lagrange_at(domain_of(nc, l), tau)
    u, v, w = [0] * m, [0] * m, [0] * m
    for acc, M in ((u, A), (v, B), (w, C)):
        for i, row in enumerate(M):
            for c, val in row:
                acc[c] = (acc[c] + val * L[i]) % R
    for j in range(l):
        u[j] = (u[j] + L[nc + j]) % R
    return u, v, w


class _FixedBase:
    """k G from a table of 2^i G"""

    def __init__(self, gen, dbl, add, zero):
        self.add, self.zero, self.table = add, zero, [gen]
        for _ in range(253):
            self.table.append(dbl(self.table[-1]))

    def mul(self, k):
        acc, i = self.zero, 0
        k %= R
        while k:
            if k & 1:
                acc = self.add(acc, self.table[i])
            k >>= 1
            i += 1
        return acc


def _g1_fixed():
    if "g1" not in _cache:
        j = _FixedBase((1, 2, 1), opy._jac_double, opy._jac_add, (1, 1, 0))
        _cache["g1"] = lambda k: _g1(opy.jac_to_affine(j.mul(k))) if k % R else None
    return _cache["g1"]


def _g2_fixed():
    if "g2" not in _cache:
        gx, gy = pr.G2_GEN
        j = _FixedBase((gx, gy, (1, 0)), g2.jac_dbl, g2.jac_add, None)
        _cache["g2"] = lambda k: g2.jac_to_affine(j.mul(k)) if k % R else None
    return _cache["g2"]


def trapdoor_scalars(matrices, l, m, trap):
    """the discrete logarithms of every point of the key: u, v, gamma_abc as the setup names them, and the dictionary closed_form_logs
    takes -- the columns a (= u), b1 and b2 (= v, both), l, h and the fixed points alpha, beta_g1 = beta_g2, delta_g1 = delta_g2"""
    tau, alpha, beta, gamma, delta = trap
    n = domain_of(len(matrices[0]), l)
    u, v, w = qap_at(matrices, l, m, tau)
    gi, di = pow(gamma, R - 2, R), pow(delta, R - 2, R)
    comb = [(beta * u[j] + alpha * v[j] + w[j]) % R for j in range(m)]
    zt = (pow(tau, n, R) - 1) * di % R
    return dict(u=u, v=v, gamma_abc=[c * gi % R for c in comb[:l]], l=[c * di % R for c in comb[l:]],
                h=[pow(tau, i, R) * zt % R for i in range(n - 1)], a=u, b1=v, b2=v, alpha=alpha, beta_g1=beta, beta_g2=beta, delta_g1=delta,
                delta_g2=delta)


def trapdoor_setup(matrices, l, m, trap):
    tau, alpha, beta, gamma, delta = trap
    sc = trapdoor_scalars(matrices, l, m, trap)
    m1, m2 = _g1_fixed(), _g2_fixed()
    return Key(alpha_g1=m1(alpha), beta_g1=m1(beta), delta_g1=m1(delta), beta_g2=m2(beta), gamma_g2=m2(gamma), delta_g2=m2(delta),
               gamma_abc_g1=[m1(x) for x in sc["gamma_abc"]], a_query=[m1(x) for x in sc["u"]], b_g1_query=[m1(x) for x in sc["v"]],
               b_g2_query=[m2(x) for x in sc["v"]], h_query=[m1(x) for x in sc["h"]], l_query=[m1(x) for x in sc["l"]])


def closed_form_sums(logs, l, z, h):
    """the part of a proof's logarithms that the blinds do not enter: the four MSMs without their delta terms, (a0, b10, b20, k0).
    logs: the logarithms of the key's points -- lists a, b1, b2 (m each), l (m - l), h (n - 1), integers alpha, beta_g1, beta_g2
    (delta_g1, delta_g2 enter with the blinds); trapdoor_scalars makes one, tests/g16_pool.py another."""
    dot = lambda xs, cs: sum(x * y for x, y in zip(xs, cs))
    assert len(logs["a"]) == len(logs["b1"]) == len(logs["b2"]) == len(z) and len(logs["l"]) == len(z) - l and len(logs["h"]) == len(h) - 1
    return ((logs["alpha"] + dot(z, logs["a"])) % R, (logs["beta_g1"] + dot(z, logs["b1"])) % R, (logs["beta_g2"] + dot(z, logs["b2"])) % R,
            (dot(z[l:], logs["l"]) + dot(h, logs["h"])) % R)


def closed_form_blind(sums, logs, r, s):
    """(a, b, c) from closed_form_sums and the blinds: a = a0 + r delta_1, b1 = b10 + s delta_1, b = b20 + s delta_2,
    c = s a + r b1 + k0 - r s delta_1"""
    a0, b10, b20, k0 = sums
    a = (a0 + r * logs["delta_g1"]) % R
    b1 = (b10 + s * logs["delta_g1"]) % R
    return a, (b20 + s * logs["delta_g2"]) % R, (s * a + r * b1 + k0 - r * s * logs["delta_g1"]) % R


def closed_form_logs(logs, l, z, r, s, h):
    """the discrete logarithms (a, b, c) of the proof under a key of known logarithms: A = a G, B = b G2, C = c G"""
    return closed_form_blind(closed_form_sums(logs, l, z, h), logs, r, s)


def closed_form(matrices, l, z, r, s, trap, h):
    """closed_form_logs for a trapdoor key"""
    return closed_form_logs(trapdoor_scalars(matrices, l, len(z), trap), l, z, r, s, h)


def points_of(a, b, c):
    return _g1_fixed()(a), _g2_fixed()(b), _g1_fixed()(c)


def verify(key, public, proof):
    """e(A, B) = e(alpha, beta) e(sum_i public_i IC_i, gamma) e(C, delta); public includes the leading one"""
    A, B, C = proof
    ic = None
    for x, pt in zip(public, key.gamma_abc_g1):
        ic = opy.g1_add(ic, opy.g1_mul(pt, x)) if pt is not None else ic
    return pr.pairing_product_is_one([(opy.g1_neg(A), B), (key.alpha_g1, key.beta_g2), (ic, key.gamma_g2), (C, key.delta_g2)])


# ---- wire formats -------------------------------------------------------------------------------------------------------------
def g1_to_wire(points):
    return oc.points_from_affine([p if p is not None else (0, 0) for p in points]).reshape(-1, 8)


def g1_from_wire(w):
    out = []
    for row in np.asarray(w, dtype=np.uint64).reshape(-1, 8):
        out.append(_g1(opy.wire_to_affine(row.tobytes())))
    return out


def proof_to_wire(proof):
    """[32] uint64: A (8), B (16), C (8)"""
    A, B, C = proof
    return np.concatenate([g1_to_wire([A])[0], g2.points_to_wire([B])[0], g1_to_wire([C])[0]])


def csr(rows):
    """(row_ptr u64, col u32, val [nnz, 4] Montgomery words)"""
    row_ptr, col, val = [0], [], []
    for r in rows:
        col += [c for c, _ in r]
        val += [v for _, v in r]
        row_ptr.append(len(col))
    return (np.array(row_ptr, dtype=np.uint64), np.array(col, dtype=np.uint32), oc.fr_from_ints(val).reshape(-1, 4))


def from_csr(row_ptr, col, val):
    v = oc.fr_to_ints(val) if len(col) else []
    return [[(int(col[k]), v[k]) for k in range(int(row_ptr[i]), int(row_ptr[i + 1]))] for i in range(len(row_ptr) - 1)]


def key_arrays(key, sy_m, l, nc, matrices):
    """the arguments of backend.Groth16Key.from_arrays"""
    return dict(n_vars=sy_m, n_inputs=l, n_constraints=nc, alpha_g1=g1_to_wire([key.alpha_g1])[0], beta_g1=g1_to_wire([key.beta_g1])[0],
                delta_g1=g1_to_wire([key.delta_g1])[0], beta_g2=g2.points_to_wire([key.beta_g2])[0], delta_g2=g2.points_to_wire([key.delta_g2])[0],
                a_query=g1_to_wire(key.a_query), b_g1_query=g1_to_wire(key.b_g1_query), l_query=g1_to_wire(key.l_query),
                h_query=g1_to_wire(key.h_query), b_g2_query=g2.points_to_wire(key.b_g2_query), matrices=[csr(M) for M in matrices])


def sha256_of(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()
