"""TEST INFRASTRUCTURE ONLY -- verify_matchmaking (matchmaking/src/build_cs.rs:101-129) -> verifier (uzkge/src/plonk/verifier.rs:17-164)
in its form WITHOUT the "shuffle" feature, over the pieces the shuffle tests already pin: the transcript of plonk_golden_verifier.py,
r_scalars / r_eval_zeta of plonk_verifier_oracle.py with shuffle=False, the pairing of oracle/bn254_pairing.py.

Against the shuffle form (plonk_golden_verifier.verify) the differences are the ones verifier.rs puts under #[cfg(feature = "shuffle")]:
no wire-selector commitments or evaluations and no q_ecc evaluation in the transcript, 19 scalars for r, and the opening at zeta over
w (5), s (4), q_prk3, q_prk4 and r.  The key is tests/golden/matchmaking_vk_golden.json in today's order of nine selectors: the file's
eight are slots 0..6 and 8, slot 7 (q_ecc, all zero in this circuit) is the identity."""
import json
import os

import bn254_py as opy
import bn254_pairing as pr
import plonk_golden_verifier as gv
import plonk_verifier_oracle as pv
from util import GOLDEN

R = opy.R
PROOF_TRANSCRIPT, N_TRANSCRIPT_PLAYERS = b"Plonk Matchmaking Proof", 50


def load_vk():
    d = json.load(open(os.path.join(GOLDEN, "matchmaking_vk_golden.json")))
    q = [gv._pt(p) for p in d["cm_q"]]
    n = int(d["cs_size"])
    root = opy.root_of_unity(n)
    return {"cm_q": q[:7] + [None] + q[7:], "cm_s": [gv._pt(p) for p in d["cm_s"]], "cm_qb": gv._pt(d["cm_qb"]),
            "cm_prk": [gv._pt(p) for p in d["cm_prk"]], "anemoi_g": int(d["anemoi_generator"]), "anemoi_g_inv": int(d["anemoi_generator_inv"]),
            "k": [int(v) for v in d["k"]], "root": root, "cs_size": n, "num_vars": int(d["num_vars"]), "pi_rows": [int(v) for v in d["pi_rows"]],
            "pi_root_powers": [pow(root, int(r), R) for r in d["pi_rows"]], "pi_lagrange": [int(v) for v in d["pi_lagrange_constants"]]}


def init_transcript(vk, pi, players):
    """verify_matchmaking's transcript up to the proof: the label, the number of inputs, transcript_init_plonk"""
    t = gv.Transcript(PROOF_TRANSCRIPT)
    t.append_u64(players)
    t.append_message(b"PLONK")
    t.append_u64(vk["cs_size"])
    t.append_message(R.to_bytes(32, "big"))
    for c in vk["cm_q"] + vk["cm_s"]:
        t.append_commitment(c)
    t.append_challenge(vk["root"])
    for k in vk["k"]:
        t.append_challenge(k)
    for v in pi:
        t.append_challenge(v)
    return t


def evaluations(proof):
    """the proof's 15 scalars in the order compute_challenges appends them (and round 4 returns them)"""
    return proof["w"] + proof["s"] + [proof["prk3"], proof["prk4"], proof["z_omega"]] + proof["w_omega"]


def verify(vk, proof, pi, players=N_TRANSCRIPT_PLAYERS, g2=None):
    """True iff the proof is accepted under the online inputs `pi` (inputs, outputs, random number, commitment)."""
    if g2 is None:
        g2 = pr.parse_srs_g2(open(os.path.join(GOLDEN, "srs-padding.bin"), "rb").read())
    n = vk["cs_size"]
    t = init_transcript(vk, pi, players)
    for c in proof["cm_w"]:
        t.append_commitment(c)
    beta = t.challenge()
    t.append_single_byte(0x01)
    gamma = t.challenge()
    t.append_commitment(proof["cm_z"])
    alpha = t.challenge()
    for c in proof["cm_t"]:
        t.append_commitment(c)
    zeta = t.challenge()
    for v in evaluations(proof):
        t.append_challenge(v)
    u = t.challenge()
    ch = {"alpha": alpha, "beta": beta, "gamma": gamma, "zeta": zeta, "anemoi_g": vk["anemoi_g"], "edwards_a": 0}
    ev = {"w": proof["w"], "s": proof["s"], "prk3": proof["prk3"], "prk4": proof["prk4"], "z_omega": proof["z_omega"], "w_omega": proof["w_omega"]}
    zh, _ = pv.first_lagrange_poly(zeta, n)
    acc = 0
    for v, c, rp in zip(pi, vk["pi_lagrange"], vk["pi_root_powers"]):
        acc += v % R * c % R * pow((zeta - rp) % R, -1, R)
    pi_eval = acc % R * zh % R
    r_eval = pv.r_eval_zeta(ch, n, ev, pi_eval, False, anemoi_g_inv=vk["anemoi_g_inv"])
    scalars = pv.r_scalars(ch, vk["k"], n, ev, False)
    bases = vk["cm_q"] + [proof["cm_z"], vk["cm_s"][4], vk["cm_qb"], vk["cm_prk"][0], vk["cm_prk"][1]] + proof["cm_t"]
    assert len(bases) == len(scalars) == 19
    cm_r = None
    for b, s in zip(bases, scalars):
        if b is not None and s:
            cm_r = opy.g1_add(cm_r, opy.g1_mul(b, s))

    def batch(cms, vals, point):                              # PolyComScheme::batch
        t.append_message(b"New PCS-Batch-Eval Protocol")
        t.append_message(R.to_bytes(32, "big"))
        t.append_u64(n + 2)
        t.append_challenge(point)
        a = t.challenge()
        c_comb, v_comb, mult = None, 0, 1
        for c, v in zip(cms, vals):
            if c is not None:
                c_comb = opy.g1_add(c_comb, opy.g1_mul(c, mult))
            v_comb = (v_comb + mult * v) % R
            mult = mult * a % R
        return c_comb, v_comb
    zeta_omega = zeta * vk["root"] % R
    cms = proof["cm_w"] + vk["cm_s"][:4] + [vk["cm_prk"][2], vk["cm_prk"][3], cm_r]
    vals = proof["w"] + proof["s"] + [proof["prk3"], proof["prk4"], r_eval]
    comm, val = batch(cms, vals, zeta)
    comm_o, val_o = batch([proof["cm_z"]] + proof["cm_w"][:3], [proof["z_omega"]] + proof["w_omega"], zeta_omega)
    # batch_verify_diff_points with the challenge u
    pi0, pi1 = proof["open_zeta"], opy.g1_mul(proof["open_zeta_omega"], u)
    left = opy.g1_add(pi0, pi1)
    right = opy.g1_add(opy.g1_mul(pi0, zeta), opy.g1_mul(pi1, zeta_omega))
    right = opy.g1_add(right, opy.g1_neg(opy.g1_mul(opy.G1_GEN, (val + u * val_o) % R)))
    right = opy.g1_add(right, opy.g1_add(comm, opy.g1_mul(comm_o, u)))
    return pr.pairing_product_is_one([(left, g2[1]), (opy.g1_neg(right), g2[0])])


class ProverTranscript:
    """The prover's side of the same transcript, driving prove_matchmaking's challenges (prover.rs:151-372)."""

    def __init__(self, vk, pi, players=N_TRANSCRIPT_PLAYERS):
        from uzkge_amd.poly_commit import fr_from_int
        self.wire, self.vk, self.ch = fr_from_int, vk, {}
        self.t = init_transcript(vk, pi, players)

    def _commitments(self, cms):
        from util import affine_of
        for j in cms:
            self.t.append_commitment(affine_of(j))

    def beta_gamma(self, cms):
        self._commitments(cms)
        self.ch["beta"] = self.t.challenge()
        self.t.append_single_byte(0x01)
        self.ch["gamma"] = self.t.challenge()
        return self.wire(self.ch["beta"]), self.wire(self.ch["gamma"])

    def alpha(self, cm_z):
        self._commitments(cm_z[:1])
        self.ch["alpha"] = self.t.challenge()
        return self.wire(self.ch["alpha"])

    def zeta(self, cm_t):
        self._commitments(cm_t)
        self.ch["zeta"] = self.t.challenge()
        return self.wire(self.ch["zeta"])

    def after_evaluations(self, rows, zeta_w, zeta_omega_w):
        for v in pv._ints(rows):                                # round 4's order is compute_challenges' order (tools/prover_chain.py eval_plan(False))
            self.t.append_challenge(v)
        self.ch["u"] = self.t.challenge()
        out = []
        for point in (zeta_w, zeta_omega_w):                    # batch_prove -> init_pcs_batch_eval_transcript + alpha (pcs.rs:107-118)
            self.t.append_message(b"New PCS-Batch-Eval Protocol")
            self.t.append_message(R.to_bytes(32, "big"))
            self.t.append_u64(self.vk["cs_size"] + 2)
            self.t.append_challenge(pv._ints(point)[0])
            out.append(self.wire(self.t.challenge()))
        return out


def evals_of(rows):
    """round 4's 15 rows as the dictionary r_scalars / r_eval_zeta take"""
    v = pv._ints(rows)
    return {"w": v[0:5], "s": v[5:9], "prk3": v[9], "prk4": v[10], "z_omega": v[11], "w_omega": v[12:15]}
