"""zshuffle's circuit and its witness on the device: deck -> remask -> witness -> five rounds, with no trace download and no host-side
circuit builder in between (include/uzkge_gpu.h, "the shuffle circuit").

    circuit = ShuffleCircuit.create(52, lagrange_bases, srs_powers, k)     # once per deck size: layout, tables, the 32 key commitments
    cm_pk = circuit.set_key(key)                                           # once per game: the 12 public-key tables from T_pk
    w = circuit.witness(key, e1, e2, digits, perms)                        # per shuffle: `batch` decks, witnesses stay on the device
    out = prove_shuffle(circuit, w, 0, fs, r_scalars_of, blinds)           # the five rounds for deck 0

As everywhere in this library the transcript, the blinds and r_poly's O(1) scalars are the caller's: `fs` answers each round's
commitments or evaluations with the next challenges, `r_scalars_of` turns round 4's evaluations into round 5's 43 scalars
(tools/prover_chain.py drives a stand-in circuit the same way)."""
import numpy as np

from . import backend as b
from . import poly_commit as pc

HIDE_W, HIDE_WSEL, HIDE_Z = (3, 3, 3, 2, 2), 2, 3                 # TurboCS::get_hiding_degree, prover.rs:186, :204


class ShuffleWitness:
    """The device-resident witnesses of `batch` decks and what came back to the host with them."""

    def __init__(self, n, batch, d_witness, d_wsel, pi_values, e1_out, e2_out):
        self.n, self.batch, self.d_witness, self.d_wsel = n, batch, d_witness, d_wsel
        self.pi_values, self.e1_out, self.e2_out = pi_values, e1_out, e2_out

    def witness_ptr(self, deck: int) -> int:
        return self.d_witness + 32 * 5 * self.n * deck

    def wsel_ptr(self, deck: int) -> int:
        return self.d_wsel + 32 * 3 * self.n * deck

    def release(self) -> None:
        for name in ("d_witness", "d_wsel"):
            if getattr(self, name):
                b.dev_free(getattr(self, name))
                setattr(self, name, 0)


class ShuffleCircuit(b.ShuffleCircuit):
    @classmethod
    def create(cls, cards: int, lagrange_bases, srs_powers, k, precompute: bool = False) -> "ShuffleCircuit":
        """lagrange_bases: the n points of the Lagrange SRS of the circuit's size; srs_powers: at least n + 3 monomial powers (the
        six that apply_blind_factors touches are taken from them); k: verifier_params.k [5, 4]."""
        n = b.shuffle_cs_info(cards)["n"]
        powers = np.ascontiguousarray(srs_powers, dtype=np.uint64).reshape(-1, 8)
        assert powers.shape[0] >= n + 3, "the blind factors need the powers n .. n + 2"
        return cls(cards, lagrange_bases, np.concatenate([powers[:3], powers[n:n + 3]]), k, precompute=precompute)

    def witness(self, key, e1, e2, digits, perms=None) -> ShuffleWitness:
        a = np.asarray(e1)
        batch = a.reshape(-1, a.shape[-2], 8).shape[0]
        d_w, d_s = b.dev_alloc(32 * 5 * self.n * batch), b.dev_alloc(32 * 3 * self.n * batch)
        try:
            pi, o1, o2 = self.witness_batch(key, e1, e2, digits, perms, d_w, d_s)
        except Exception:
            b.dev_free(d_w)
            b.dev_free(d_s)
            raise
        return ShuffleWitness(self.n, batch, d_w, d_s, pi, o1, o2)


def prove_shuffle(circuit: ShuffleCircuit, witness: ShuffleWitness, deck: int, fs, r_scalars_of, blinds, prover: b.Prover = None) -> dict:
    """One deck's proof from its device witness.
      fs            beta_gamma(cm_w_wsel) -> (beta, gamma); alpha(cm_z); zeta(cm_t); after_evaluations(evals, zeta, zeta_omega) ->
                    (alpha_zeta, alpha_zeta_omega): the caller's transcript, elements as [4] Montgomery words
      r_scalars_of  evals [19, 4] -> [43, 4]: r_poly's scalars (helpers.rs:681-1002)
      blinds        dict: "w" [5, 3, 4], "wsel" [3, 3, 4] (unused third slots zero), "z" [3, 4], "t" [5, 4]
    Returns cm_w_wsel [8, 12], cm_z [1, 12], cm_t [5, 12], evals [19, 4], openings [2, 12]: a PlonkProof's 14 + 2 points and 19 scalars."""
    own = prover is None
    pr = b.Prover(circuit.n, 1, shared=False) if own else prover
    try:
        o = {}
        o["cm_w_wsel"] = pr.round1(circuit, witness.witness_ptr(deck), witness.wsel_ptr(deck), circuit.pi_rows, witness.pi_values[deck:deck + 1],
                                   list(HIDE_W) + [HIDE_WSEL] * 3, np.concatenate([blinds["w"], blinds["wsel"]]), on_device=True)
        beta, gamma = fs.beta_gamma(o["cm_w_wsel"])
        o["cm_z"] = pr.round2(beta, gamma, blinds["z"])
        o["cm_t"] = pr.round3(fs.alpha(o["cm_z"]), blinds["t"])
        zeta = fs.zeta(o["cm_t"])
        o["evals"] = pr.round4(zeta, True)
        zeta_omega = pc.fr_from_int(pc.fr_to_int(np.asarray(zeta).reshape(4)) * pc.fr_to_int(b.domain_group_gen(circuit.n)) % pc.FR_MODULUS)
        a0, a1 = fs.after_evaluations(o["evals"], zeta, zeta_omega)
        o["openings"] = pr.round5(r_scalars_of(o["evals"]), a0, a1)
        return o
    finally:
        if own:
            pr.destroy()
