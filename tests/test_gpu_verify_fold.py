"""GPU: uzk_verify_fold (csrc/verify.hip) held to tests/plonk_batch_ref.py, with the oracle pairing as the final verdict.

The device decodes the proof bytes, runs the Keccak transcripts, derives the verifier scalars and folds m proofs into the two points
of one pairing check.  Compared here: the Keccak sponge alone (test hook), the seven challenges, both points against the Python fold,
the verdict of the pairing for good batches and for every class of alteration, the status codes of malformed input, proofs made by
this library's own prover (distinct proofs under one key, with and without the shuffle feature), and the Python mirror."""
import copy
import os
import sys

import numpy as np
import pytest

import bn254_py as opy
import oracle_c as oc
import plonk_batch_ref as br
import plonk_golden_verifier as gv
import plonk_verifier_oracle as pv
from util import affine_of

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

R, P = opy.R, opy.P


@pytest.fixture(scope="module")
def g2():
    return br.load_g2()


@pytest.fixture(scope="module")
def golden52(gpu):
    from uzkge_amd.poly_commit import PlonkVerifierKey
    vk, proof, pi = gv.load_golden(52)
    key = PlonkVerifierKey(vk, br.prefix(52))
    left, right = br.fold([br.terms(vk, proof, pi, br.prefix(52))], [1])
    yield {"vk": vk, "proof": proof, "pi": pi, "key": key, "raw": gv.proof_to_bytes(proof), "left": left, "right": right}
    key.release()


def _weights(m, seed):
    rng = np.random.default_rng(seed)
    w = [int.from_bytes(rng.bytes(16), "little") | 1 for _ in range(m)]
    assert len(set(w)) == m
    return w


def _raw_fold(key, proofs, pis, weights, want_challenges=False):
    """the raw call: wire arrays in, (left, right) as affine integer points, status, [challenges as integers]"""
    from uzkge_amd.poly_commit import fr_from_int, fr_to_int
    m = len(proofs)
    pi = np.stack([np.stack([fr_from_int(v) for v in row]) for row in pis]) if key.n_pi and m else np.zeros((m, key.n_pi, 4), dtype=np.uint64)
    w = None if weights is None else np.stack([fr_from_int(v) for v in weights])
    out = key.key.fold(b"".join(proofs), pi, w, want_challenges=want_challenges)
    res = (affine_of(out[0]), affine_of(out[1]), [int(s) for s in out[2]])
    if want_challenges:
        res += ([[fr_to_int(c) for c in row] for row in out[3]],)
    return res


def test_keccak_hook_matches_the_restatement(gpu):
    rng = np.random.default_rng(11)
    msgs = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (0, 1, 31, 32, 33, 135, 136, 137, 271, 272, 273, 14600)]
    msgs += [b"abc", b"\x00" * 136, b"\xff" * 135]
    got = gpu.keccak256_device(msgs)
    assert got[12].hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    for m, d in zip(msgs, got):
        assert d == gv.keccak256(m), len(m)
    many = [bytes([i & 255]) * (i % 300) for i in range(200)]                  # more messages than one workgroup has lanes
    assert gpu.keccak256_device(many) == [gv.keccak256(m) for m in many]


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("cards", [52, 20])
def test_one_golden_proof_with_weight_one(gpu, g2, cards, form):
    """m = 1, NULL weights: the seven challenges, both points and the verdict -- and the round trip of the bytes.  form: the
    transcript kernel (0 the default choice, 1 one proof per lane, 2 a proof's sponge state spread over a half wave)."""
    from uzkge_amd.poly_commit import PlonkVerifierKey
    vk, proof, pi = gv.load_golden(cards)
    key = PlonkVerifierKey(vk, br.prefix(cards))
    gpu.tune("verify_transcript", form)
    try:
        assert key.key.info()[:3] == (vk["cs_size"], 8 * cards, 1632)
        raw = gv.proof_to_bytes(proof)
        left, right, status, ch = _raw_fold(key, [raw], [pi], None, want_challenges=True)
        assert status == [0]
        assert ch[0] == br.challenges(vk, proof, pi, br.prefix(cards))
        want = br.fold([br.terms(vk, proof, pi, br.prefix(cards))], [1])
        assert (left, right) == want
        assert br.accepts(left, right, g2) and gv.verify(vk, gv.proof_from_bytes(raw), pi, n_cards=cards, g2=g2)
        # an explicit weight of 1 is the same call; another weight scales both points
        assert _raw_fold(key, [raw], [pi], [1])[:2] == want
        l7, r7, _ = _raw_fold(key, [raw], [pi], [7])
        assert (l7, r7) == (opy.g1_mul(want[0], 7), opy.g1_mul(want[1], 7))
        # the empty batch
        l0, r0, s0 = _raw_fold(key, [], [], None)
        assert l0 is None and r0 is None and s0 == []
    finally:
        gpu.tune("verify_transcript", 0)
        key.release()


@pytest.mark.parametrize("m", [3, 70])
def test_both_transcript_kernels_give_the_same_challenges(gpu, golden52, m):
    """Different proofs in one batch (copies with one evaluation changed each, and one refused proof in the middle): the two forms of
    the transcript kernel agree on every challenge, and with the restatement on the first and the last proof."""
    g = golden52
    proofs, raws = [], []
    for i in range(m):
        p = copy.deepcopy(g["proof"]); p["s"][i % 4] = (p["s"][i % 4] + i) % R
        proofs.append(p); raws.append(gv.proof_to_bytes(p))
    raws[1] = raws[1][:32 * 33] + R.to_bytes(32, "big") + raws[1][32 * 34:]
    weights = _weights(m, 3)
    out = {}
    try:
        for form in (1, 2):
            gpu.tune("verify_transcript", form)
            out[form] = _raw_fold(g["key"], raws, [g["pi"]] * m, weights, want_challenges=True)
    finally:
        gpu.tune("verify_transcript", 0)
    assert out[1][2] == out[2][2] == [0, 1] + [0] * (m - 2)
    assert out[1][:2] == out[2][:2]
    for i in range(m):
        if i != 1:
            assert out[1][3][i] == out[2][3][i], i
    for i in (0, m - 1):
        assert out[2][3][i] == br.challenges(g["vk"], proofs[i], g["pi"], br.prefix(52))


def _altered(g, what):
    """(proof bytes, public inputs) of the golden proof with one thing changed"""
    proof, pi = copy.deepcopy(g["proof"]), list(g["pi"])
    if what == "evaluation":
        proof["w"][3] = (proof["w"][3] + 1) % R
    elif what == "commitment":
        proof["cm_t"][2] = opy.g1_add(proof["cm_t"][2], opy.G1_GEN)
    elif what == "public_input":
        pi[100] = (pi[100] + 1) % R
    elif what == "witness":
        proof["open_zeta"] = opy.g1_add(proof["open_zeta"], opy.G1_GEN)
    return gv.proof_to_bytes(proof), pi


@pytest.mark.parametrize("m", [64, 1024])
def test_copies_under_distinct_weights(gpu, g2, golden52, m):
    g = golden52
    weights = _weights(m, 100 + m)
    left, right, status = _raw_fold(g["key"], [g["raw"]] * m, [g["pi"]] * m, weights)
    assert status == [0] * m
    total = sum(weights) % R
    assert left == opy.g1_mul(g["left"], total) and right == opy.g1_mul(g["right"], total)
    assert br.accepts(left, right, g2)
    rng = np.random.default_rng(m)
    for what in ("evaluation", "commitment", "public_input", "witness"):
        at = int(rng.integers(0, m))
        raw, pi = _altered(g, what)
        proofs, pis = [g["raw"]] * m, [g["pi"]] * m
        proofs[at], pis[at] = raw, pi
        l, r, status = _raw_fold(g["key"], proofs, pis, weights)
        assert status == [0] * m
        assert (l, r) != (left, right) and not br.accepts(l, r, g2), what
    # the public-key commitments of another game: every proof is rejected; the right ones again: accepted
    pk = list(g["vk"]["cm_shuffle_public_key"])
    other = list(pk); other[5] = opy.g1_add(pk[5], opy.G1_GEN)
    g["key"].set_public_key(other)
    try:
        l, r, _ = _raw_fold(g["key"], [g["raw"]] * m, [g["pi"]] * m, weights)
        assert not br.accepts(l, r, g2)
        l1, r1, _ = _raw_fold(g["key"], [g["raw"]], [g["pi"]], None)
        assert not br.accepts(l1, r1, g2)
        vk2 = dict(g["vk"], cm_shuffle_public_key=other)
        assert (l1, r1) == br.fold([br.terms(vk2, g["proof"], g["pi"], br.prefix(52))], [1])
    finally:
        g["key"].set_public_key(pk)
    assert _raw_fold(g["key"], [g["raw"]] * m, [g["pi"]] * m, weights)[:2] == (left, right)


def test_malformed_input(gpu, g2, golden52):
    g = golden52
    raw = g["raw"]
    word = lambda blob, i, v: blob[:32 * i] + int(v).to_bytes(32, "big") + blob[32 * (i + 1):]
    y0 = int.from_bytes(raw[32:64], "big")
    coord_p = word(raw, 20, P)                                   # a coordinate of cm_t[2] equal to p
    scalar_r = word(raw, 33, R)                                  # w[3] equal to r
    off_curve = word(raw, 1, (y0 + 1) % P)                       # cm_w[0] with y + 1
    top = word(raw, 46, (1 << 256) - 1)                          # all ones
    weights = _weights(6, 5)
    proofs = [raw, coord_p, raw, scalar_r, off_curve, top]
    left, right, status = _raw_fold(g["key"], proofs, [g["pi"]] * 6, weights)
    assert status == [0, 1, 0, 1, 2, 1]
    good = br.terms(g["vk"], g["proof"], g["pi"], br.prefix(52))
    assert (left, right) == br.fold([good, good], [weights[0], weights[2]])
    assert br.accepts(left, right, g2)
    # a single bad proof: nothing is folded
    l, r, status = _raw_fold(g["key"], [off_curve], [g["pi"]], None)
    assert status == [2] and l is None and r is None
    # a commitment of zeros is the point at infinity: decoded, folded, and the batch is rejected by the pairing
    proof = copy.deepcopy(g["proof"]); proof["cm_wsel"][1] = None
    inf = gv.proof_to_bytes(proof)
    assert inf[32 * 12:32 * 14] == bytes(64)
    l, r, status = _raw_fold(g["key"], [raw, inf], [g["pi"]] * 2, weights[:2])
    assert status == [0, 0]
    assert (l, r) == br.fold([good, br.terms(g["vk"], proof, g["pi"], br.prefix(52))], weights[:2])
    assert not br.accepts(l, r, g2)


def test_python_mirror_returns_the_raw_call(gpu, g2, golden52):
    g = golden52
    weights = _weights(3, 9)
    left, right, status = g["key"].fold([g["raw"]] * 3, [g["pi"]] * 3, weights)
    assert list(status) == [0, 0, 0] and left.shape == (12,) and right.shape == (12,)
    assert (affine_of(left), affine_of(right)) == _raw_fold(g["key"], [g["raw"]] * 3, [g["pi"]] * 3, weights)[:2]
    l1, r1, _ = g["key"].fold([g["raw"]], [g["pi"]])
    assert (affine_of(l1), affine_of(r1)) == (g["left"], g["right"]) and br.accepts(affine_of(l1), affine_of(r1), g2)
    from uzkge_amd import UzkgeError
    with pytest.raises(UzkgeError) as e:
        g["key"].fold([g["raw"]] * 2, [g["pi"]] * 2)            # a batch without weights
    assert e.value.kind == "ParameterError"
    with pytest.raises(UzkgeError):
        g["key"].fold([g["raw"][:-1]], [g["pi"]])


# ---- proofs made by this library's prover -----------------------------------------------------------------------------------------
class _FiatShamir:
    """The prover's side of the reference's transcript (prover.rs:151-372 appends what verifier.rs:166-222 re-derives), driving the
    chain's challenges -- tests/test_gpu_plonk_verifier.py's, with the order of a circuit without the shuffle feature added."""

    def __init__(self, vk, pi, prefix, plan, shuffle):
        from uzkge_amd.poly_commit import fr_from_int
        self.wire, self.plan, self.vk, self.ch, self.shuffle = fr_from_int, plan, vk, {}, shuffle
        t = gv.Transcript.__new__(gv.Transcript)
        t.state = bytes(prefix)
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
        self.t = t

    def beta_gamma(self, cms):
        # the chain commits its wire-selector vectors whatever the circuit is; a proof without the shuffle feature has cm_w only
        for j in cms if self.shuffle else cms[:5]:
            self.t.append_commitment(affine_of(j))
        self.ch["beta"] = self.t.challenge()
        self.t.append_single_byte(0x01)
        self.ch["gamma"] = self.t.challenge()
        return self.wire(self.ch["beta"]), self.wire(self.ch["gamma"])

    def alpha(self, cm_z):
        self.t.append_commitment(affine_of(cm_z[0]))
        self.ch["alpha"] = self.t.challenge()
        return self.wire(self.ch["alpha"])

    def zeta(self, cm_t):
        for j in cm_t:
            self.t.append_commitment(affine_of(j))
        self.ch["zeta"] = self.t.challenge()
        return self.wire(self.ch["zeta"])

    def after_evaluations(self, rows, zeta_w, zeta_omega_w):
        import prover_chain as pch
        v = pv._ints(rows)
        at = {(kind, idx, pt): i for i, (kind, idx, pt) in enumerate(self.plan)}
        order = [("c", i, 0) for i in range(5)] + [("t", pch.T_S + i, 0) for i in range(4)]
        if self.shuffle:
            order += [("c", 5 + i, 0) for i in range(3)]
        order += [("t", pch.T_QPRK + 2, 0), ("t", pch.T_QPRK + 3, 0), ("c", 9, 1)]
        if self.shuffle:
            order += [("t", pch.T_QECC, 0)]
        order += [("c", i, 1) for i in range(3)]
        for key in order:
            self.t.append_challenge(v[at[key]])
        self.ch["u"] = self.t.challenge()
        out = []
        for point in (zeta_w, zeta_omega_w):
            self.t.append_message(b"New PCS-Batch-Eval Protocol")
            self.t.append_message(R.to_bytes(32, "big"))
            self.t.append_u64(self.vk["cs_size"] + 2)
            self.t.append_challenge(pv._ints(point)[0])
            out.append(self.wire(self.t.challenge()))
        return out


def _prove(n, shuffle, count, prefix):
    """`count` proofs of one satisfiable circuit with different blinds: (vk, g1_0, [(proof dict, proof bytes)], pi)"""
    import prover_chain as pch
    from uzkge_amd import backend as b
    from util import rand_fr_wire
    inp = pv.make_satisfiable(pch.ChainInputs(n, 21), seed=4)
    c = pch.ProverChain(inputs=inp, precompute=False, shuffle=shuffle)
    try:
        table_cms = [affine_of(j) for j in b.msm_batch(c.srs, b.ntt_batch(inp.table_polys))]
        omega = pv._ints(inp.group_gen)[0]
        ninv = pow(n, -1, R)
        g = pv._ints(inp.anemoi_g)[0]
        vk = {"cm_q": table_cms[pch.T_Q:pch.T_Q + 9], "cm_s": table_cms[pch.T_S:pch.T_S + 5], "cm_qb": table_cms[pch.T_QB],
              "cm_prk": table_cms[pch.T_QPRK:pch.T_QPRK + 4], "cm_q_ecc": table_cms[pch.T_QECC],
              "cm_shuffle_generator": table_cms[pch.T_QG:pch.T_QG + 12], "cm_shuffle_public_key": table_cms[pch.T_QPK:pch.T_QPK + 12],
              "anemoi_g": g, "anemoi_g_inv": pow(g, -1, R), "k": pv._ints(inp.k), "edwards_a": pv._ints(inp.edwards_a)[0],
              "root": omega, "cs_size": n, "pi_root_powers": [pow(omega, j, R) for j in range(8)],
              "pi_lagrange": [pow(omega, j, R) * ninv % R for j in range(8)]}
        g1_0 = opy.wire_to_affine(inp.mono_wire[0].tobytes())
        vk["g1_0"] = g1_0
        pi = pv._ints(inp.pi_evals[:8])
        plan = pch.eval_plan(shuffle)
        at = {(kind, idx, pt): i for i, (kind, idx, pt) in enumerate(plan)}
        k = vk["k"]

        def evals_of(rows):
            v = pv._ints(rows)
            ev = {"w": [v[at[("c", i, 0)]] for i in range(5)], "s": [v[at[("t", pch.T_S + i, 0)]] for i in range(4)],
                  "prk3": v[at[("t", pch.T_QPRK + 2, 0)]], "prk4": v[at[("t", pch.T_QPRK + 3, 0)]], "z_omega": v[at[("c", 9, 1)]],
                  "w_omega": [v[at[("c", i, 1)]] for i in range(3)]}
            if shuffle:
                ev["q_ecc"] = v[at[("t", pch.T_QECC, 0)]]
                ev["wsel"] = [v[at[("c", 5 + i, 0)]] for i in range(3)]
            return ev
        proofs = []
        for j in range(count):
            fs = _FiatShamir(vk, pi, prefix, plan, shuffle)
            c.fs = fs
            chd = lambda: {"alpha": fs.ch["alpha"], "beta": fs.ch["beta"], "gamma": fs.ch["gamma"], "zeta": fs.ch["zeta"], "anemoi_g": g,
                           "edwards_a": vk["edwards_a"]}
            c.r_scalar_hook = lambda rows: oc.fr_from_ints(pv.r_scalars(chd(), k, n, evals_of(rows), shuffle))
            if j:                                               # other blinds: another proof of the same statement
                bw = rand_fr_wire(15, 1000 + j).reshape(5, 3, 4)
                bw[c.blinds_w.reshape(5, 3, 4).any(axis=2) == 0] = 0           # the unused third slots stay zero
                c.blinds_w = bw
                c.blinds_z = rand_fr_wire(c.blinds_z.shape[0], 2000 + j)
                c.t_rands = rand_fr_wire(5, 3000 + j)
            o = c.run()
            ev = evals_of(o["evals"])
            proof = {"cm_w": [affine_of(x) for x in o["cm_w_wsel"][:5]], "cm_t": [affine_of(x) for x in o["cm_t"]], "cm_z": affine_of(o["cm_z"][0]),
                     "prk3": ev["prk3"], "prk4": ev["prk4"], "w": ev["w"], "w_omega": ev["w_omega"], "z_omega": ev["z_omega"], "s": ev["s"],
                     "open_zeta": affine_of(o["cm_q"][0]), "open_zeta_omega": affine_of(o["cm_q"][1])}
            if shuffle:
                proof.update(cm_wsel=[affine_of(x) for x in o["cm_w_wsel"][5:8]], q_ecc=ev["q_ecc"], wsel=ev["wsel"])
            proofs.append((proof, _to_bytes(proof, shuffle)))
        return vk, g1_0, proofs, pi
    finally:
        c.release()


def _to_bytes(proof, shuffle):
    """PlonkProof::to_bytes_be with and without the shuffle members (indexer.rs:539-590)"""
    if shuffle:
        return gv.proof_to_bytes(proof)
    pt = lambda p: b"".join(int(v).to_bytes(32, "big") for v in ((0, 0) if p is None else p))
    sc = lambda v: (v % R).to_bytes(32, "big")
    out = b"".join(pt(p) for p in proof["cm_w"] + proof["cm_t"] + [proof["cm_z"]])
    out += sc(proof["prk3"]) + sc(proof["prk4"]) + b"".join(sc(v) for v in proof["w"] + proof["w_omega"]) + sc(proof["z_omega"])
    out += b"".join(sc(v) for v in proof["s"])
    return out + pt(proof["open_zeta"]) + pt(proof["open_zeta_omega"])


def test_distinct_proofs_under_one_key(gpu, g2):
    """Four proofs of one satisfiable circuit (n = 2^14, anemoi rounds and the quintic selector live) with different blinds, made by
    the round API, folded in one call: accepted, equal to the Python fold; one of them altered: rejected."""
    from uzkge_amd.poly_commit import PlonkVerifierKey
    prefix = br.prefix(52)
    vk, g1_0, proofs, pi = _prove(1 << 14, True, 4, prefix)
    assert len({raw for _, raw in proofs}) == 4 and all(len(raw) == 1632 for _, raw in proofs)
    assert gv.verify(vk, proofs[1][0], pi, n_cards=52, g2=g2)                  # g1_0 of these parameters is the generator
    assert g1_0 == opy.G1_GEN
    key = PlonkVerifierKey(vk, prefix, g1_0=g1_0)
    try:
        weights = _weights(4, 77)
        left, right, status = _raw_fold(key, [raw for _, raw in proofs], [pi] * 4, weights)
        assert status == [0] * 4
        assert (left, right) == br.fold([br.terms(vk, p, pi, prefix) for p, _ in proofs], weights)
        assert br.accepts(left, right, g2)
        bad = copy.deepcopy(proofs[2][0]); bad["s"][1] = (bad["s"][1] + 1) % R
        raws = [raw for _, raw in proofs]; raws[2] = gv.proof_to_bytes(bad)
        l, r, _ = _raw_fold(key, raws, [pi] * 4, weights)
        assert not br.accepts(l, r, g2)
    finally:
        key.release()


def test_a_proof_without_the_shuffle_feature(gpu, g2):
    """A circuit of n = 2^13 without wire selectors (zmatchmaking's shape): 1312-byte proofs under a shuffle = 0 key."""
    from uzkge_amd.poly_commit import PlonkVerifierKey
    prefix = br.prefix(52)
    vk, g1_0, proofs, pi = _prove(1 << 13, False, 1, prefix)
    proof, raw = proofs[0]
    assert len(raw) == 1312
    key = PlonkVerifierKey(vk, prefix, g1_0=g1_0, shuffle=False)
    try:
        assert key.key.info()[:3] == (1 << 13, 8, 1312)
        left, right, status, ch = _raw_fold(key, [raw], [pi], None, want_challenges=True)
        assert status == [0]
        assert ch[0] == br.challenges(vk, proof, pi, prefix, shuffle=False)
        assert (left, right) == br.fold([br.terms(vk, proof, pi, prefix, shuffle=False)], [1])
        assert br.accepts(left, right, g2)
        bad = copy.deepcopy(proof); bad["w_omega"][1] = (bad["w_omega"][1] + 1) % R
        l, r, _ = _raw_fold(key, [_to_bytes(bad, False)], [pi], None)
        assert not br.accepts(l, r, g2)
        from uzkge_amd import UzkgeError
        with pytest.raises(UzkgeError):
            key.set_public_key([None] * 12)                     # no public-key commitments in such a key
    finally:
        key.release()
