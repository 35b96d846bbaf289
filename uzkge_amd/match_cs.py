"""zmatchmaking's circuit and its witness on the device: match -> hash and stream cipher -> witness -> five rounds, with no trace
download and no host-side circuit builder in between (include/uzkge_gpu.h, "the matchmaking circuit").

    circuit = MatchCircuit.create(50, lagrange_bases, srs_powers, k)       # once per player count: layout, tables, the 19 key commitments
    w = circuit.witness(inputs, seeds, randoms)                            # per batch of matches: witnesses stay on the device
    out = prove_matchmaking(circuit, w, 0, fs, r_scalars_of, blinds)       # the five rounds for match 0

As everywhere in this library the transcript, the blinds and r_poly's O(1) scalars are the caller's: `fs` answers each round's
commitments or evaluations with the next challenges, `r_scalars_of` turns round 4's evaluations into round 5's 19 scalars.  The
reference's transcript is "Plonk Matchmaking Proof" with append_u64("Number inputs", players)."""
import numpy as np

from . import backend as b
from . import poly_commit as pc

HIDE_W, HIDE_Z = (3, 3, 3, 2, 2), 3                                # TurboCS::get_hiding_degree, prover.rs:204


class MatchWitness:
    """The device-resident witnesses of `batch` matches and what came back to the host with them."""

    def __init__(self, n, batch, d_witness, pi_values, outputs, commitments):
        self.n, self.batch, self.d_witness = n, batch, d_witness
        self.pi_values, self.outputs, self.commitments = pi_values, outputs, commitments

    def witness_ptr(self, match: int) -> int:
        return self.d_witness + 32 * 5 * self.n * match

    def release(self) -> None:
        if self.d_witness:
            b.dev_free(self.d_witness)
            self.d_witness = 0


class MatchCircuit(b.MatchCircuit):
    @classmethod
    def create(cls, players: int, lagrange_bases, srs_powers, k, precompute: bool = False) -> "MatchCircuit":
        """lagrange_bases: the n points of the Lagrange SRS of the circuit's size; srs_powers: at least n + 3 monomial powers (the
        six that apply_blind_factors touches are taken from them); k: verifier_params.k [5, 4]."""
        n = b.match_cs_info(players)["n"]
        powers = np.ascontiguousarray(srs_powers, dtype=np.uint64).reshape(-1, 8)
        assert powers.shape[0] >= n + 3, "the blind factors need the powers n .. n + 2"
        return cls(players, lagrange_bases, np.concatenate([powers[:3], powers[n:n + 3]]), k, precompute=precompute)

    def witness(self, inputs, seeds, randoms) -> MatchWitness:
        a = np.asarray(inputs)
        batch = a.reshape(-1, a.shape[-2], 4).shape[0]
        d_w = b.dev_alloc(32 * 5 * self.n * max(batch, 1))
        try:
            pi, out, cm = self.witness_batch(inputs, seeds, randoms, d_w)
        except Exception:
            b.dev_free(d_w)
            raise
        return MatchWitness(self.n, batch, d_w, pi, out, cm)


def prove_matchmaking(circuit: MatchCircuit, witness: MatchWitness, match: int, fs, r_scalars_of, blinds, prover: b.Prover = None) -> dict:
    """One match's proof from its device witness.
      fs            beta_gamma(cm_w) -> (beta, gamma); alpha(cm_z); zeta(cm_t); after_evaluations(evals, zeta, zeta_omega) ->
                    (alpha_zeta, alpha_zeta_omega): the caller's transcript, elements as [4] Montgomery words
      r_scalars_of  evals [15, 4] -> [19, 4]: r_poly's scalars without the shuffle feature (helpers.rs:681-1002)
      blinds        dict: "w" [5, 3, 4] (unused third slots zero), "z" [3, 4], "t" [5, 4]
    Returns cm_w [5, 12], cm_z [1, 12], cm_t [5, 12], evals [15, 4], openings [2, 12]: a PlonkProof's 11 + 2 points and 15 scalars."""
    own = prover is None
    pr = b.Prover(circuit.n, 1, shared=False) if own else prover
    try:
        o = {}
        o["cm_w"] = pr.round1(circuit, witness.witness_ptr(match), None, circuit.pi_rows, witness.pi_values[match:match + 1], list(HIDE_W), blinds["w"],
                              on_device=True)
        beta, gamma = fs.beta_gamma(o["cm_w"])
        o["cm_z"] = pr.round2(beta, gamma, blinds["z"])
        o["cm_t"] = pr.round3(fs.alpha(o["cm_z"]), blinds["t"])
        zeta = fs.zeta(o["cm_t"])
        o["evals"] = pr.round4(zeta, False)
        zeta_omega = pc.fr_from_int(pc.fr_to_int(np.asarray(zeta).reshape(4)) * pc.fr_to_int(b.domain_group_gen(circuit.n)) % pc.FR_MODULUS)
        a0, a1 = fs.after_evaluations(o["evals"], zeta, zeta_omega)
        o["openings"] = pr.round5(r_scalars_of(o["evals"]), a0, a1)
        return o
    finally:
        if own:
            pr.destroy()
