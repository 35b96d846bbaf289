"""TEST INFRASTRUCTURE ONLY -- the batch form of the verifier of tests/plonk_golden_verifier.py on Python integers.

`gv.verify` ends in  e(left, [tau] G2) = e(right, G2)  with left and right sums of (base, scalar) products.  `terms` flattens one
proof's two sides into those products -- every commitment of the key and of the proof once, r(X)'s scalars (plonk_verifier_oracle
r_scalars) times the power of the batch challenge that cm_r carries -- and `fold` adds the sides of several proofs under one weight
each:  L = sum rho_i left_i,  R = sum rho_i right_i.  With weights nobody can predict the folded equation holds only if every
proof's own equation does.  uzk_verify_fold (csrc/verify.hip) is held to these two functions; the pairing stays outside both.

  prefix(n_cards)                          the caller's transcript bytes before transcript_init_plonk (verify_shuffle)
  challenges(vk, proof, pi, prefix, shuffle)   beta, gamma, alpha, zeta, u and the two PolyComScheme::batch challenges
  terms(vk, proof, pi, prefix, shuffle)    ([(base, scalar)] of the left side, [(base, scalar)] of the right side)
  fold(cases, weights)                     (L, R) as affine points (None = infinity); cases = [(left_terms, right_terms)]
  accepts(L, R, g2)                        the pairing check

Only tests import this file."""
import os

import bn254_py as opy
import bn254_pairing as pr
import plonk_golden_verifier as gv
import plonk_verifier_oracle as pv
from util import GOLDEN

R = opy.R


def prefix(n_cards):
    t = gv.Transcript(b"Plonk shuffle Proof")
    t.append_u64(n_cards)
    return t.state


def load_g2():
    return pr.parse_srs_g2(open(os.path.join(GOLDEN, "srs-padding.bin"), "rb").read())


def _evaluations(proof, shuffle):
    ev = {"w": proof["w"], "s": proof["s"], "prk3": proof["prk3"], "prk4": proof["prk4"], "z_omega": proof["z_omega"], "w_omega": proof["w_omega"]}
    if shuffle:
        ev["q_ecc"], ev["wsel"] = proof["q_ecc"], proof["wsel"]
    return ev


def _run(vk, proof, pi, prefix_bytes, shuffle):
    """The transcript and the scalar side of gv.verify; returns the challenges and the two term lists."""
    n = vk["cs_size"]
    t = gv.Transcript.__new__(gv.Transcript)
    t.state = bytes(prefix_bytes)
    t.append_message(b"PLONK")                                  # transcript_init_plonk
    t.append_u64(n)
    t.append_message(R.to_bytes(32, "big"))
    for c in vk["cm_q"] + vk["cm_s"]:
        t.append_commitment(c)
    t.append_challenge(vk["root"])
    for k in vk["k"]:
        t.append_challenge(k)
    for v in pi:
        t.append_challenge(v)
    wsel_cms = proof["cm_wsel"] if shuffle else []
    for c in proof["cm_w"] + wsel_cms:                          # compute_challenges
        t.append_commitment(c)
    beta = t.challenge()
    t.append_single_byte(0x01)
    gamma = t.challenge()
    t.append_commitment(proof["cm_z"])
    alpha = t.challenge()
    for c in proof["cm_t"]:
        t.append_commitment(c)
    zeta = t.challenge()
    tail = (proof["wsel"] if shuffle else []) + [proof["prk3"], proof["prk4"], proof["z_omega"]] + ([proof["q_ecc"]] if shuffle else [])
    for v in proof["w"] + proof["s"] + tail + proof["w_omega"]:
        t.append_challenge(v)
    u = t.challenge()
    ch = {"alpha": alpha, "beta": beta, "gamma": gamma, "zeta": zeta, "anemoi_g": vk["anemoi_g"], "edwards_a": vk["edwards_a"]}
    ev = _evaluations(proof, shuffle)
    zh, _ = pv.first_lagrange_poly(zeta, n)
    acc = 0                                                     # eval_pi_poly with the key's own constants
    for v, c, rp in zip(pi, vk["pi_lagrange"], vk["pi_root_powers"]):
        acc += v % R * c % R * pow((zeta - rp) % R, -1, R)
    pi_eval = acc % R * zh % R
    r_eval = pv.r_eval_zeta(ch, n, ev, pi_eval, shuffle, anemoi_g_inv=vk["anemoi_g_inv"])
    scalars = pv.r_scalars(ch, vk["k"], n, ev, shuffle)
    r_bases = vk["cm_q"] + [proof["cm_z"], vk["cm_s"][4], vk["cm_qb"], vk["cm_prk"][0], vk["cm_prk"][1]]
    if shuffle:
        r_bases += vk["cm_shuffle_public_key"] + vk["cm_shuffle_generator"]
    r_bases += proof["cm_t"]
    assert len(r_bases) == len(scalars) == (43 if shuffle else 19)

    def batch_challenge(point):                                 # init_pcs_batch_eval_transcript + the challenge of PolyComScheme::batch
        t.append_message(b"New PCS-Batch-Eval Protocol")
        t.append_message(R.to_bytes(32, "big"))
        t.append_u64(n + 2)
        t.append_challenge(point)
        return t.challenge()
    zeta_omega = zeta * vk["root"] % R
    a = batch_challenge(zeta)
    b = batch_challenge(zeta_omega)
    cms = proof["cm_w"] + vk["cm_s"][:4] + [vk["cm_prk"][2], vk["cm_prk"][3]]
    vals = proof["w"] + proof["s"] + [proof["prk3"], proof["prk4"]]
    if shuffle:
        cms += [vk["cm_q_ecc"]] + proof["cm_wsel"]
        vals += [proof["q_ecc"]] + proof["wsel"]
    right, val, mult = [], 0, 1
    for c, v in zip(cms, vals):                                 # a^j for the j-th commitment opened at zeta
        right.append((c, mult))
        val = (val + mult * v) % R
        mult = mult * a % R
    right += [(base, mult * s % R) for base, s in zip(r_bases, scalars)]       # a^J s_k for the bases of r(X)
    val = (val + mult * r_eval) % R
    val_o, mult = 0, 1
    for c, v in zip([proof["cm_z"]] + proof["cm_w"][:3], [proof["z_omega"]] + proof["w_omega"]):
        right.append((c, u * mult % R))                         # u b^j at zeta omega
        val_o = (val_o + mult * v) % R
        mult = mult * b % R
    right.append((vk.get("g1_0", opy.G1_GEN), (-(val + u * val_o)) % R))
    right.append((proof["open_zeta"], zeta))
    right.append((proof["open_zeta_omega"], u * zeta_omega % R))
    left = [(proof["open_zeta"], 1), (proof["open_zeta_omega"], u)]
    return [beta, gamma, alpha, zeta, u, a, b], left, right


def challenges(vk, proof, pi, prefix_bytes, shuffle=True):
    return _run(vk, proof, pi, prefix_bytes, shuffle)[0]


def terms(vk, proof, pi, prefix_bytes, shuffle=True):
    _, left, right = _run(vk, proof, pi, prefix_bytes, shuffle)
    return left, right


def _sum(pairs, weight):
    """sum weight * scalar * base with the scalars of one base added first"""
    by_base = {}
    for base, s in pairs:
        if base is not None:
            by_base[base] = (by_base.get(base, 0) + weight * s) % R
    return by_base


def fold(cases, weights):
    """cases: [(left_terms, right_terms)]; weights: one Fr integer each.  Returns (L, R) as affine points (None = infinity)."""
    assert len(cases) == len(weights)
    out = []
    for side in (0, 1):
        total = {}
        for case, rho in zip(cases, weights):
            for base, s in _sum(case[side], rho % R).items():
                total[base] = (total.get(base, 0) + s) % R
        acc = None
        for base, s in total.items():
            if s:
                acc = opy.g1_add(acc, opy.g1_mul(base, s))
        out.append(acc)
    return out[0], out[1]


def accepts(left, right, g2):
    """e(L, [tau] G2) = e(R, G2)"""
    return pr.pairing_product_is_one([(left, g2[1]), (opy.g1_neg(right), g2[0])])
