"""GPU: zmatchmaking's circuit and its witness on the device (uzk_match_circuit_create, uzk_match_witness_batch), held to
tests/match_cs_ref.py -- which tests/test_match_cs_ref_host.py holds to the verifier key the reference ships for 50 players -- and, at
50 players, to that key directly and to the verifier restated without the shuffle feature (tests/match_verifier.py): proofs made from
the device witness over the literal circuit are accepted under the reference's own commitments and the online inputs the witness call
returned, and under no others."""
import ctypes
import random

import numpy as np
import pytest

import anemoi_ref as an
import match_cs_ref as mr
import match_verifier as mv
import oracle_c as oc
import plonk_verifier_oracle as pv
from test_gpu_shuffle_cs import bases, root_of, wire
from test_match_cs_ref_host import built, golden_key, golden_vk, match
from util import affine_of

pytestmark = pytest.mark.gpu
R = mr.R


def make_circuit(players, k=None):
    from uzkge_amd import backend as b
    from uzkge_amd.match_cs import MatchCircuit
    lag, mono = bases(b.match_cs_info(players)["n"])
    k = [1, 2, 3, 4, 5] if k is None else k                 # any five distinct cosets serve the layout tests
    return MatchCircuit.create(players, lag, mono, oc.fr_from_ints(k))


@pytest.fixture(scope="module")
def literal(gpu):
    """the literal circuit of the reference's 50 players under the reference's k"""
    vk = mv.load_vk()
    cir = make_circuit(50, vk["k"])
    yield dict(vk=vk, cir=cir)
    cir.release()


@pytest.fixture(scope="module")
def bound(gpu):
    """the circuit of UZK_MATCH_CS_MAX_PLAYERS players: the only one of 16384 rows, with 22 permutation blocks"""
    from uzkge_amd import _native as N
    assert N.MATCH_CS_MAX_PLAYERS == mr.MAX_PLAYERS == 64
    cir = make_circuit(N.MATCH_CS_MAX_PLAYERS)
    yield cir
    cir.release()


ROWS = {50: 8192, 63: 8192, 64: 16384}               # 63 players are the most that fit 8192 rows (8054 gates; 64 have 8295)


@pytest.mark.parametrize("players", [3, 5, 8, 50, 63, 64])
def test_wiring_permutation_and_every_evaluation_vector(gpu, players):
    k = [1, 7, 13, 17, 23]
    cir = make_circuit(players, k)
    try:
        cs = built(players, zero=True)
        n = cs.size
        assert n == ROWS.get(players, n)
        info = gpu.match_cs_info(players)
        assert (info["size"], info["n"], info["num_vars"], info["pi_count"]) == (cs.gates, n, cs.num_vars, 2 * players + 2)
        assert cir.info()[:3] == (n, 15, 19)                 # a circuit without the shuffle feature
        assert info["pi_rows"].tolist() == cs.public_vars_constraint_indices
        wiring, perm, evals = cir.test_tables()
        assert wiring.reshape(-1).tolist() == [v for w in cs.wiring for v in w]
        assert perm.reshape(-1).tolist() == mr.compute_permutation(cs)
        want = mr.key_vectors(cs, k, root_of(n))
        assert len(want) == evals.shape[0] == 19
        for i, vec in enumerate(want):
            assert np.array_equal(evals[i], wire(vec)), "vector %d" % i
        assert not evals[7].any() and evals[15:].any()       # q_ecc is zero, the round keys are not
    finally:
        cir.release()


def test_the_key_commitments_are_the_golden_verifier_key(gpu, literal):
    cir, vk = literal["cir"], literal["vk"]
    assert root_of(cir.n) == vk["root"] and cir.n == vk["cs_size"] == 8192 and cir.num_vars == vk["num_vars"]
    assert cir.pi_rows.tolist() == vk["pi_rows"]
    got = [affine_of(j) for j in cir.commitments]
    assert len(got) == 19 and got[7] is None                 # the 19th of today's order, q_ecc, is the identity
    assert [None if g is None else list(g) for g in got] == golden_key(golden_vk())


def fr_rows(values):
    return oc.fr_from_ints([v % R for v in values])


def matches_wire(ms):
    return (np.stack([fr_rows(m[0]) for m in ms]), fr_rows([m[1] for m in ms]), fr_rows([m[2] for m in ms]))


def expect(m):
    cs = mr.build_cs(*m)
    pi = mr.public_inputs(cs)
    n = len(m[0])
    return wire([v for w in mr.extend_witness(cs) for v in w]), wire(pi), wire(pi[n:2 * n]), wire([an.eval_variable_length_hash([m[1]])])[0]


def run_witness(gpu, cir, ms):
    w = cir.witness(*matches_wire(ms))
    try:
        return gpu.dev_download(w.d_witness, (len(ms), 5 * cir.n, 4)), w.pi_values, w.outputs, w.commitments
    finally:
        w.release()


def edge_match(players, kind):
    """all zero (gen_prover_params' match), or every element r - 1"""
    v = 0 if kind == "zero" else R - 1
    return [v] * players, v, v


def check_witness(gpu, cir, ms, alone=0):
    """every lane of one call against the restatement; the rows behind the pad; lane `alone` in a call of its own"""
    got = run_witness(gpu, cir, ms)
    for lane, m in enumerate(ms):
        for name, g, w in zip(("witness", "pi", "outputs", "commitment"), got, expect(m)):
            assert np.array_equal(g[lane], w), (lane, name)
    ext = got[0].reshape(len(ms), 5, cir.n, 4)
    assert not ext[:, :, cir.size:].any()                    # the rows behind the pad hold variable 0's value: zero
    # alone, a match gives what it gives inside a batch
    single = run_witness(gpu, cir, ms[alone:alone + 1])
    assert all(np.array_equal(a[0], b[alone]) for a, b in zip(single, got))
    return got


@pytest.mark.parametrize("players,batch", [(3, 65), (5, 7), (8, 7), (50, 3), (63, 3)])
def test_witness_inputs_outputs_and_commitments_are_the_restated_ones(gpu, literal, players, batch):
    ms = [match(players, 40 + i) for i in range(batch)]
    ms[1] = edge_match(players, "zero")
    if batch > 3:
        ms[2] = edge_match(players, "max")
        ms[3] = (list(range(players)), ms[3][1], ms[3][2])   # distinct small inputs: the outputs are a visible permutation
    cir = literal["cir"] if players == 50 else make_circuit(players)
    try:
        got = check_witness(gpu, cir, ms)
        if batch > 3:
            assert sorted(oc.fr_to_ints(got[2][3])) == list(range(players))
    finally:
        if players != 50:
            cir.release()


def test_witness_at_the_player_bound(gpu, bound):
    """64 players: the whole wave divides and walks (divisors 2 .. 64, 63 steps, the last reads lane 63), the state table has 65
    rows, the cipher runs 21 permutations and the circuit 16384 rows.  One call holds the all-zero match, the all-(r - 1) match, the
    match of the inputs 0 .. 63 and a random one."""
    players = mr.MAX_PLAYERS
    assert (bound.players, bound.n, bound.size) == (players, 16384, 8295)
    ms = [match(players, 60 + i) for i in range(4)]
    ms[0], ms[1] = edge_match(players, "zero"), edge_match(players, "max")
    ms[2] = (list(range(players)), ms[2][1], ms[2][2])
    got = check_witness(gpu, bound, ms, alone=3)
    outs = oc.fr_to_ints(got[2][2])
    assert sorted(outs) == list(range(players)) and outs != list(range(players))
    # what came out is the Fisher-Yates walk of all 63 steps on plain integers
    stream, want = an.eval_stream_cipher([ms[2][1], ms[2][2]], players - 1), list(range(players))
    for i in range(1, players):
        r = stream[i - 1] % (i + 1)
        want[i], want[r] = want[r], want[i]
    assert outs == want


def test_every_case_of_the_first_middle_and_last_steps_at_the_player_bound(gpu, bound):
    """The matches of tests/test_match_cs_bounds.py, which that module shows to take the self-exchange rem_i == i, the exchange with
    position 0 and an exchange in between at each of the steps 1, 31, 32, 62 and 63 of the walk at 64 players."""
    from test_match_cs_bounds import directed_matches, wanted
    ms, seen, _ = directed_matches()
    assert seen == wanted()
    check_witness(gpu, bound, ms, alone=len(ms) - 1)


def plain_words(values):
    return np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in values], dtype=np.uint64)


def test_the_kernels_division_is_divmod(gpu):
    for m in range(2, 65):
        values = [0, m - 1, m, R - 1, (R - 1) // m * m]
        for k in range(1, 8):
            values += [(1 << (32 * k)) - 1, 1 << (32 * k), (1 << (32 * k)) + 1]
        assert all(v < R for v in values)
        q, r = gpu.match_divrem(plain_words(values), m)
        got = [(sum(int(w) << (64 * i) for i, w in enumerate(row)), int(rem)) for row, rem in zip(q, r)]
        assert got == [divmod(v, m) for v in values], "m = %d" % m


def test_refusals_leave_the_circuit_usable(gpu):
    from uzkge_amd import UzkgeError
    from uzkge_amd import _native as N
    from test_gpu_shuffle_cs import make_circuit as make_shuffle_circuit
    import shuffle_ref as sr
    from test_shuffle_cs_ref_host import game
    players = 3
    cir, other, shuffle = make_circuit(players), make_circuit(4), make_shuffle_circuit(3)
    n = cir.n
    d_w = gpu.dev_alloc(32 * 5 * max(n, shuffle.n))
    d_s = gpu.dev_alloc(32 * 3 * shuffle.n)
    poison = np.full((5 * n, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    plain = gpu.Circuit(16, bases(4096)[0][:16], bases(4096)[1][:6], np.arange(80, dtype=np.uint32), oc.fr_from_ints([1, 2, 3, 4, 5]), np.zeros(4, dtype=np.uint64),
                        np.zeros(4, dtype=np.uint64), oc.fr_from_ints([1])[0], [None] * 46)
    good = match(players, 77)
    want = expect(good)
    inputs, seeds, randoms = matches_wire([good])
    over = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)       # the words of r itself
    try:
        def still_usable():
            got = run_witness(gpu, cir, [good])
            assert all(np.array_equal(g[0], w) for g, w in zip(got, want))

        def refused(circuit=cir, a=inputs, s=seeds, r=randoms):
            gpu.dev_upload(d_w, poison)
            with pytest.raises(UzkgeError) as err:
                gpu.MatchCircuit.witness_batch(circuit, a, s, r, d_w)
            assert err.value.code == N.UZK_ERR_PARAMETER, str(err.value)
            assert np.array_equal(gpu.dev_download(d_w, (5 * n, 4)), poison)
            still_usable()
            return str(err.value)
        still_usable()
        plain.players = shuffle.players = players
        assert "no circuit of uzk_match_circuit_create" in refused(circuit=plain)
        assert "no circuit of uzk_match_circuit_create" in refused(circuit=shuffle)
        assert "matches of 3 players, the circuit is for 4" in refused(circuit=other)
        assert "0 matches" in refused(a=inputs[:0], s=seeds[:0], r=randoms[:0])
        too_many = N.MATCH_CS_MAX_BATCH + 1
        assert "%d matches" % too_many in refused(a=np.repeat(inputs, too_many, axis=0), s=np.repeat(seeds, too_many, axis=0), r=np.repeat(randoms, too_many, axis=0))
        for which in range(3):
            bad = [inputs.copy(), seeds.copy(), randoms.copy()]
            bad[which].reshape(-1, 4)[-1] = over
            assert "not below r" in refused(a=bad[0], s=bad[1], r=bad[2])
        # a null pointer in every position
        pi, out, cm = np.zeros((2 * players + 2, 4), dtype=np.uint64), np.zeros((players, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
        vp = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
        args = [vp(inputs), vp(seeds), vp(randoms), players, 1, ctypes.c_void_p(d_w), vp(pi), vp(out), vp(cm)]
        for at in (0, 1, 2, 5, 6, 7, 8):
            call = list(args)
            call[at] = None
            assert gpu.lib.uzk_match_witness_batch(cir.handle, *call) == N.UZK_ERR_PARAMETER
            still_usable()
        # the shuffle's entry points refuse a matchmaking circuit, and go on serving their own
        pk, deck, digits, perm = game(3, 41)
        e1 = np.stack([sr.e.points_wire([c[0] for c in deck])])
        e2 = np.stack([sr.e.points_wire([c[1] for c in deck])])
        with gpu.RemarkKey(sr.e.points_wire([pk])[0]) as key:
            cir.cards = 3
            for call in (lambda: gpu.ShuffleCircuit.witness_batch(cir, key, e1, e2, np.array([digits], dtype=np.uint8), None, d_w, d_s),
                         lambda: gpu.ShuffleCircuit.set_key(cir, key)):
                with pytest.raises(UzkgeError) as err:
                    call()
                assert err.value.code == N.UZK_ERR_PARAMETER and "no circuit of uzk_shuffle_circuit_create" in str(err.value)
            shuffle.set_key(key)
            shuffle.witness_batch(key, e1, e2, np.array([digits], dtype=np.uint8), None, d_w, d_s)
        still_usable()
        for bad in (0, 2, 65):
            with pytest.raises(UzkgeError):
                gpu.match_cs_info(bad)
    finally:
        gpu.dev_free(d_w)
        gpu.dev_free(d_s)
        for c in (plain, cir, other, shuffle):
            c.release()


def blinds(seed):
    rng = random.Random(seed)
    fr = lambda *shape: oc.fr_from_ints([rng.randrange(R) for _ in range(int(np.prod(shape)))]).reshape(shape + (4,))
    bl = {"w": fr(5, 3), "z": fr(3), "t": fr(5)}
    bl["w"][3:, 2] = 0
    return bl


def prove(cir, w, lane, vk, seed):
    """one proof through uzkge_amd.match_cs.prove_matchmaking: (PlonkProof as a dict, the online inputs it was made under)"""
    from uzkge_amd.match_cs import prove_matchmaking
    pi = pv._ints(w.pi_values[lane])
    t = mv.ProverTranscript(vk, pi, cir.players)
    ch = lambda: dict(t.ch, anemoi_g=vk["anemoi_g"], edwards_a=0)
    o = prove_matchmaking(cir, w, lane, t, lambda rows: oc.fr_from_ints(pv.r_scalars(ch(), vk["k"], vk["cs_size"], mv.evals_of(rows), False)), blinds(seed))
    ev = mv.evals_of(o["evals"])
    proof = dict(ev, cm_w=[affine_of(j) for j in o["cm_w"]], cm_t=[affine_of(j) for j in o["cm_t"]], cm_z=affine_of(o["cm_z"][0]),
                 open_zeta=affine_of(o["openings"][0]), open_zeta_omega=affine_of(o["openings"][1]))
    return proof, pi


def test_proofs_from_the_device_witness_are_accepted_under_the_golden_key(gpu, literal):
    import plonk_batch_ref as br
    cir, vk = literal["cir"], literal["vk"]
    g2 = br.load_g2()
    ms = [(list(range(1000, 1050)), 11, 12), match(50, 91)]
    w = cir.witness(*matches_wire(ms))
    try:
        (p0, pi0), (p1, pi1) = prove(cir, w, 0, vk, 5), prove(cir, w, 1, vk, 6)
        outs = pi0[50:100]
        assert pi0[:50] == ms[0][0] and sorted(outs) == ms[0][0] and pi0[100:] == [12, an.eval_variable_length_hash([11])]
        assert p0["prk3"] != 0 and len(p0["cm_w"]) == 5      # the Anemoi rows are live; no wire selectors
        assert mv.verify(vk, p0, pi0, g2=g2) and mv.verify(vk, p1, pi1, g2=g2)
        assert not mv.verify(vk, p0, pi1, g2=g2) and not mv.verify(vk, p1, pi0, g2=g2)
        i, j = next((i, j) for i in range(50) for j in range(i + 1, 50) if outs[i] != outs[j])
        swapped = list(pi0)
        swapped[50 + i], swapped[50 + j] = outs[j], outs[i]
        assert not mv.verify(vk, p0, swapped, g2=g2)         # one output swapped in the online inputs
    finally:
        w.release()
