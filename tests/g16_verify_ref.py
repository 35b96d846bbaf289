"""CPU restatement of the batch Groth16 verification of include/uzkge_gpu.h (uzk_g16_vk_create / uzk_g16_verify_fold) on Python
integers: the 256-byte proof blob, the status rules, the fold and its pairing product, and a SIMULATOR that makes valid proofs for a
trapdoor key without running a prover.

  parse_blob / make_blob   eight 32-byte big-endian words in the EVM order a.x, a.y, b.x.c1, b.x.c0, b.y.c1, b.y.c0, c.x, c.y
  status_of                0 decoded; 1 a word >= p; 2 A or C off y^2 = x^3 + 3 or B off the twist; 3 B on the twist, [r] B != O
  fold                     a_i = rho_i A_i, b_i = B_i, (sum rho) alpha, sum rho_i X_i, sum rho_i C_i over the proofs with status 0
  product_is_one           the M + 3 Miller loops and the final exponentiation (oracle/bn254_pairing.py)
  trapdoor_vk / simulate   a key whose discrete logs are known, and (a G, b G2, c G) with c = (a b - alpha beta - gamma sum x_j ic_j) / delta

G1 points are affine integer tuples (x, y), G2 points ((x0, x1), (y0, y1)); None = infinity (all-zero words on the wire)."""
import hashlib
import json
import os
import random

import numpy as np

import g16_ref as gr
import g2_ref as g2

pr, opy = gr.pr, gr.opy
R, P = gr.R, gr.P
GOLDEN_JSON = os.path.join(gr.GOLDEN, "groth16_reveal_golden.json")
GOLDEN_SHA256 = "7b36f1adc622a88f4aece9b1b51580b05fe2627ee4e81b723195e2c73d3eee16"
VK_BYTES = 456                                    # of groth16-reveal-head.bin
PROOF_BYTES = 256
OK, NOT_CANONICAL, OFF_CURVE, NOT_IN_SUBGROUP = 0, 1, 2, 3


# ---- the blob -----------------------------------------------------------------------------------------------------------------
def make_blob_words(w):
    assert len(w) == 8
    return b"".join(int(v).to_bytes(32, "big") for v in w)


def proof_words(proof):
    A, B, C = proof
    a, c = A or (0, 0), C or (0, 0)
    (bx0, bx1), (by0, by1) = B or ((0, 0), (0, 0))
    return [a[0], a[1], bx1, bx0, by1, by0, c[0], c[1]]


def make_blob(proof):
    return make_blob_words(proof_words(proof))


def parse_blob(blob):
    """the eight words as integers (not reduced, not checked)"""
    assert len(blob) == PROOF_BYTES
    return [int.from_bytes(blob[32 * k:32 * k + 32], "big") for k in range(8)]


def points_of_words(w):
    """(A, B, C) of eight canonical words; all-zero coordinates = None"""
    A = None if w[0] == 0 and w[1] == 0 else (w[0], w[1])
    B = None if not any(w[2:6]) else ((w[3], w[2]), (w[5], w[4]))
    C = None if w[6] == 0 and w[7] == 0 else (w[6], w[7])
    return A, B, C


def g2_mul(q, k):
    """[k] q for any point of the twist (the group law does not need the subgroup)"""
    fin = lambda t: None if t is None or t[2] == (0, 0) else t       # g2_ref doubles a point of order two into Z = 0
    acc, base = None, (q[0], q[1], (1, 0)) if q is not None else None
    while k and base is not None:
        if k & 1:
            acc = fin(g2.jac_add(acc, base))
        base = fin(g2.jac_dbl(base))
        k >>= 1
    return g2.jac_to_affine(acc) if acc is not None else None


def g2_in_subgroup(q):
    return q is None or g2_mul(q, R) is None


def status_of(blob):
    w = parse_blob(blob)
    if any(v >= P for v in w):
        return NOT_CANONICAL
    A, B, C = points_of_words(w)
    if not opy.g1_is_on_curve(A) or not opy.g1_is_on_curve(C) or not g2.g2_on_curve(B):
        return OFF_CURVE
    if not g2_in_subgroup(B):
        return NOT_IN_SUBGROUP
    return OK


# ---- the fold -----------------------------------------------------------------------------------------------------------------
def x_of(key, public):
    """sum_j x_j IC_j with x_0 = 1; public: the l - 1 inputs"""
    acc = None
    for x, pt in zip([1] + list(public), key.gamma_abc_g1):
        if pt is not None:
            acc = opy.g1_add(acc, opy.g1_mul(pt, x % R))
    return acc


def fold(key, blobs, publics, weights=None):
    """dict(a, b, alpha, x, c, status): lists of m points, three points, m status bytes"""
    m = len(blobs)
    assert weights is not None or m <= 1, "unweighted sums let errors cancel"
    weights = [1] * m if weights is None else [w % R for w in weights]
    assert len(publics) == m and len(weights) == m
    out = dict(a=[], b=[], status=[], alpha=None, x=None, c=None)
    total, t = 0, [0] * (len(key.gamma_abc_g1) - 1)
    for blob, pub, rho in zip(blobs, publics, weights):
        st = status_of(blob)
        out["status"].append(st)
        if st != OK:
            out["a"].append(None); out["b"].append(None)
            continue
        A, B, C = points_of_words(parse_blob(blob))
        out["a"].append(opy.g1_mul(A, rho) if A is not None and rho else None)
        out["b"].append(B)
        out["c"] = opy.g1_add(out["c"], opy.g1_mul(C, rho)) if C is not None and rho else out["c"]
        total = (total + rho) % R
        t = [(acc + rho * x) % R for acc, x in zip(t, pub)]
    out["alpha"] = opy.g1_mul(key.alpha_g1, total) if total else None
    out["x"] = x_of_scalars(key, [total] + t)
    return out


def x_of_scalars(key, t):
    acc = None
    for s, pt in zip(t, key.gamma_abc_g1):
        if pt is not None and s % R:
            acc = opy.g1_add(acc, opy.g1_mul(pt, s % R))
    return acc


def product_is_one(key, a, b, alpha, x, c):
    """prod e(a_i, b_i) . e(-alpha, beta) . e(-x, gamma) . e(-c, delta) == 1; pairs with a point at infinity contribute one"""
    pairs = [(p, q) for p, q in zip(a, b) if p is not None and q is not None]
    for p, q in ((alpha, key.beta_g2), (x, key.gamma_g2), (c, key.delta_g2)):
        if p is not None and q is not None:
            pairs.append((opy.g1_neg(p), q))
    return pr.pairing_product_is_one(pairs)


def accepts(key, f):
    return product_is_one(key, f["a"], f["b"], f["alpha"], f["x"], f["c"])


# ---- keys ---------------------------------------------------------------------------------------------------------------------
_cache = {}


def real_vk():
    """the verifying key of the reference's reveal circuit: the first 456 bytes of the head fixture"""
    if "vk" not in _cache:
        data = open(gr.HEAD, "rb").read()[:VK_BYTES]
        k = gr.Key()
        k.alpha_g1 = g2.decompress_g1(data[0:32])
        k.beta_g2, k.gamma_g2, k.delta_g2 = (g2.decompress_g2(data[32 + 64 * i:96 + 64 * i]) for i in range(3))
        n = int.from_bytes(data[224:232], "little")
        assert 232 + 32 * n == VK_BYTES
        k.gamma_abc_g1 = [g2.decompress_g1(data[232 + 32 * j:264 + 32 * j]) for j in range(n)]
        _cache["vk"] = k
    return _cache["vk"]


def golden():
    """(public signals, proof) of the reference's golden reveal case"""
    d = json.load(open(GOLDEN_JSON))
    return [int(v) for v in d["public_signals"]], points_of_words([int(v) for v in d["proof_words"]])


def trapdoor_vk(l, seed, ic=None):
    """(key, trap): a verifying key with l points in gamma_abc_g1 from known alpha, beta, gamma, delta and discrete logs ic_j (what
    g16_ref.trapdoor_setup makes of a constraint system, cut down to the verifier's part; `ic` fixes the logs, zeros included)"""
    rng = random.Random(f"g16-verify-trapdoor-{l}-{seed}")
    alpha, beta, gamma, delta = (rng.randrange(1, R) for _ in range(4))
    ic = [rng.randrange(1, R) for _ in range(l)] if ic is None else [v % R for v in ic]
    assert len(ic) == l
    m1, m2 = gr._g1_fixed(), gr._g2_fixed()
    key = gr.Key(alpha_g1=m1(alpha), beta_g2=m2(beta), gamma_g2=m2(gamma), delta_g2=m2(delta), gamma_abc_g1=[m1(v) for v in ic])
    return key, dict(alpha=alpha, beta=beta, gamma=gamma, delta=delta, ic=ic)


def simulate(trap, a, b, public):
    """a valid proof for ANY a, b != 0 and public inputs: (a G, b G2, c G), c = (a b - alpha beta - gamma sum_j x_j ic_j) / delta"""
    xs = sum(x * v for x, v in zip([1] + list(public), trap["ic"])) % R
    c = (a * b - trap["alpha"] * trap["beta"] - trap["gamma"] * xs) * pow(trap["delta"], R - 2, R) % R
    return gr._g1_fixed()(a), gr._g2_fixed()(b), gr._g1_fixed()(c)


def simulated_batch(trap, m, seed):
    """(proofs, publics) of m valid proofs"""
    rng = random.Random(f"g16-verify-batch-{seed}")
    l = len(trap["ic"])
    proofs, publics = [], []
    for _ in range(m):
        pub = [rng.randrange(R) for _ in range(l - 1)]
        proofs.append(simulate(trap, rng.randrange(1, R), rng.randrange(1, R), pub))
        publics.append(pub)
    return proofs, publics


# ---- points of the twist outside the subgroup -------------------------------------------------------------------------------------
def twist_point(seed):
    """a point of the twist from a seeded x (its order divides r (2 p - r): almost never r)"""
    rng = random.Random(f"g16-verify-twist-{seed}")
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = g2.f2_sqrt(g2.f2_add(g2.f2_mul(g2.f2_sqr(x), x), g2.B2))
        if y is not None:
            return (x, y)


def g2_add(p, q):
    j = lambda t: None if t is None else (t[0], t[1], (1, 0))
    s = g2.jac_add(j(p), j(q))
    return g2.jac_to_affine(s) if s is not None else None


# ---- wire forms of the expected outputs ---------------------------------------------------------------------------------------------
def a_wire(points):
    return gr.g1_to_wire(points) if points else np.zeros((0, 8), dtype=np.uint64)


def b_wire(points):
    return g2.points_to_wire(points) if points else np.zeros((0, 16), dtype=np.uint64)


def publics_wire(publics, l):
    if not publics or l == 1:
        return np.zeros((len(publics), 0, 4), dtype=np.uint64)
    return gr.oc.fr_from_ints([v for row in publics for v in row]).reshape(len(publics), l - 1, 4)


def weights_wire(weights):
    return gr.oc.fr_from_ints([w % R for w in weights]).reshape(-1, 4)


def jac_point(wire12):
    """a Jacobian wire point [12] as an affine integer point (None = infinity)"""
    w = np.asarray(wire12, dtype=np.uint64).reshape(12)
    x, y, z = (opy.from_mont(opy.limbs_to_int([int(v) for v in w[4 * k:4 * k + 4]]), P) for k in range(3))
    if z == 0:
        return None
    zi = pow(z, P - 2, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def key_wire(key):
    """the arguments of backend.Groth16VerifierKey"""
    return (gr.g1_to_wire([key.alpha_g1])[0], g2.points_to_wire([key.beta_g2])[0], g2.points_to_wire([key.gamma_g2])[0],
            g2.points_to_wire([key.delta_g2])[0], gr.g1_to_wire(key.gamma_abc_g1))


def sha256_of(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


# ---- crafted blobs of the status rules -------------------------------------------------------------------------------------------
def crafted(trap, seed=0):
    """[(name, blob, public, expected status)]: one valid proof of `trap`'s key bent in each way the status rules name.  The status-0
    entries stay valid proofs only where B is untouched; all of them are well-formed."""
    rng = random.Random(f"g16-verify-crafted-{seed}")
    l = len(trap["ic"])
    pub = [rng.randrange(R) for _ in range(l - 1)]
    good = simulate(trap, rng.randrange(1, R), rng.randrange(1, R), pub)
    w = proof_words(good)
    cases = []

    def put(name, words, status):
        cases.append((name, make_blob_words(words), pub, status))

    for k, name in ((0, "a.x = p"), (3, "b.x.c0 = p"), (7, "c.y = p")):
        put(name, w[:k] + [P] + w[k + 1:], NOT_CANONICAL)
    put("a.x = p and C off the curve", [P] + w[1:7] + [(w[7] + 1) % P], NOT_CANONICAL)        # the first check that fails
    y = next(v for v in range(1, 100) if (v * v - (P - 1) ** 3 - 3) % P)
    put("x = p - 1, y off the curve", [P - 1, y] + w[2:], OFF_CURVE)
    put("A off the curve", [w[0], (w[1] + 1) % P] + w[2:], OFF_CURVE)
    put("C off the curve", w[:7] + [(w[7] + 1) % P], OFF_CURVE)
    put("B off the twist", w[:5] + [(w[5] + 1) % P] + w[6:], OFF_CURVE)
    tw = twist_point(seed)
    assert g2.g2_on_curve(tw) and g2_mul(tw, R) is not None
    put("a random point of the twist", w[:2] + proof_words((None, tw, None))[2:6] + w[6:], NOT_IN_SUBGROUP)
    t = g2_mul(tw, R)                                              # in the cofactor's part of the twist's group
    qt = g2_add(good[1], t)
    assert g2.g2_on_curve(qt) and g2_mul(qt, R) is not None
    put("Q + T, T of cofactor order", w[:2] + proof_words((None, qt, None))[2:6] + w[6:], NOT_IN_SUBGROUP)
    for k in (1, 2, R - 1):
        put("B = %s G2" % ("r - 1" if k == R - 1 else k), w[:2] + proof_words((None, gr._g2_fixed()(k), None))[2:6] + w[6:], OK)
    return cases


# ---- the fold of simulated proofs in closed form -------------------------------------------------------------------------------------
def simulated_logs(trap, count, seed):
    """[(a, b, c, public)]: the discrete logarithms of `count` valid proofs (simulate's formula) and their public inputs"""
    rng = random.Random(f"g16-verify-logs-{seed}")
    l, di = len(trap["ic"]), pow(trap["delta"], R - 2, R)
    out = []
    for _ in range(count):
        pub = [rng.randrange(R) for _ in range(l - 1)]
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        xs = sum(x * v for x, v in zip([1] + pub, trap["ic"])) % R
        out.append((a, b, (a * b - trap["alpha"] * trap["beta"] - trap["gamma"] * xs) * di % R, pub))
    return out


def proof_of_logs(entry):
    a, b, c, _ = entry
    return gr._g1_fixed()(a), gr._g2_fixed()(b), gr._g1_fixed()(c)


def fold_logs(trap, entries, weights):
    """the fold of well-formed proofs given by their logarithms, without a group operation per proof: the logarithms of a_i and of
    the three sums, then one fixed-base multiplication each.  dict(a_log, alpha, x, c)"""
    g = gr._g1_fixed()
    total = sum(weights) % R
    t = [total] + [sum(w * e[3][j] for w, e in zip(weights, entries)) % R for j in range(len(trap["ic"]) - 1)]
    return dict(a_log=[w * e[0] % R for w, e in zip(weights, entries)], alpha=g(total * trap["alpha"] % R),
                x=g(sum(s * v for s, v in zip(t, trap["ic"])) % R), c=g(sum(w * e[2] for w, e in zip(weights, entries)) % R))
