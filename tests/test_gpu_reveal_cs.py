"""GPU: the reveal circuit (uzk_reveal_*) against tests/reveal_cs_ref.py, the restatement on Python integers: the assignments bit for
bit, the statements against uzk_cp_reveal_prove_batch, proofs accepted under the verifying key of the reference's own proving key
(tests/golden/groth16-reveal-*.bin), and every refusal.

One call has ONE secret (a player reveals cards under its key), so an edge scalar is the sk of a call of its own, and the edge points
are placed first, last and on both sides of a wave boundary of each batch.  Reference assignments are computed once per (sk, point)
from a pool of distinct points and shared."""
import ctypes
import random

import numpy as np
import pytest

import ed_ref as ed
import g16_ref as gr
import g16_verify_ref as vr
import oracle_c as oc
import reveal_cs_ref as rc

pytestmark = pytest.mark.gpu
Q = rc.Q
_rng = random.Random("gpu-reveal-cs")
ORDER8 = ed.add(ed.order8_point(), ed.mul(_rng.randrange(1, ed.L), ed.G))        # a point of order 8 times a subgroup point
EDGE_POINTS = [ed.G, ORDER8, ed.IDENTITY]
POOL = [ed.mul(_rng.randrange(1, ed.L), ed.G) for _ in range(13)]
SK = _rng.randrange(1, ed.L)
LOW128 = ((_rng.randrange(ed.L) >> 128) << 128) | ((1 << 128) - 1)
EDGE_SKS = {"0": 0, "1": 1, "l-1": ed.L - 1, "low128": LOW128}
_ref = {}


def ref_witness(sk, p):
    if (sk, p) not in _ref:
        _ref[(sk, p)] = oc.fr_from_ints(rc.witness(sk, p)).reshape(rc.N_VARS, 4)
    return _ref[(sk, p)]


def batch_points(m):
    """m points of the pool, neighbours distinct; the edge points first, last and at lanes 63 and 64 where the batch reaches them"""
    pts = [POOL[i % len(POOL)] for i in range(m)]
    places = [0, m - 1, 63, 64]
    for k, at in enumerate(places):
        if 0 <= at < m:
            pts[at] = EDGE_POINTS[k % len(EDGE_POINTS)]
    return pts


@pytest.fixture(scope="module")
def circuit(gpu):
    from uzkge_amd import reveal_cs
    data = open(gr.HEAD, "rb").read() + open(gr.g2.FIXTURE, "rb").read() + open(gr.TAIL, "rb").read()
    c = reveal_cs.RevealCircuit.from_key_bytes(data)
    yield c
    c.release()


@pytest.fixture(scope="module")
def vk(gpu):
    dk = gpu.Groth16VerifierKey(*vr.key_wire(vr.real_vk()))
    yield dk
    dk.release()


def _verify(dk, blobs, publics, seed=0):
    w = None if len(blobs) == 1 else vr.weights_wire([random.Random(f"reveal-cs-w-{seed}-{i}").randrange(1, 1 << 128) for i in range(len(blobs))])
    accepted, status = dk.verify_batch(b"".join(blobs), vr.publics_wire(publics, dk.n_inputs), w)
    return accepted, [int(s) for s in status]


_mul = {}


def ref_mul(sk, p):
    """the integer multiple [sk] p on the whole curve: no reduction of sk, p of any order"""
    if (sk, p) not in _mul:
        _mul[(sk, p)] = ed.mul(sk, p)
    return _mul[(sk, p)]


def check_batch(gpu, circuit, sk, pts, cross=True):
    """cross: the statements against uzk_cp_reveal_prove_batch too, whose contract is a secret below L"""
    from uzkge_amd import reveal as rv
    w = circuit.witness(sk, pts)
    try:
        z = w.download()
        for i, p in enumerate(pts):
            want = ref_witness(sk, p)
            if not np.array_equal(z[i], want):
                bad = [j for j in range(rc.N_VARS) if not np.array_equal(z[i, j], want[j])]
                raise AssertionError("card %d: %d variables differ, the first %d (%s)" % (i, len(bad), bad[0], rc.roles().get(bad[0])))
        if cross:
            reveal, pk, _ = gpu.cp_reveal_prove_batch(rv.scalars_to_wire([sk])[0], rv.points_to_wire(pts), rv.scalars_to_wire([7 + i for i in range(len(pts))]))
        for i in range(len(pts)):
            assert np.array_equal(w.statements_wire[i, 0:2].reshape(8), rv.points_to_wire(pts[i:i + 1])[0])
            if cross:
                assert np.array_equal(w.statements_wire[i, 2:4].reshape(8), reveal[i]) and np.array_equal(w.statements_wire[i, 4:6].reshape(8), pk)
            assert w.statements[i] == rc.witness_statement([int(v) for v in oc.fr_to_ints(ref_witness(sk, pts[i])[:7])])
            assert w.statements[i] == tuple(pts[i]) + tuple(ref_mul(sk, pts[i])) + tuple(ref_mul(sk, ed.G))
    finally:
        w.release()


def test_info_and_matrices_are_the_restatement(gpu):
    info = gpu.reveal_cs_info()
    assert (info["n_vars"], info["n_inputs"], info["n_constraints"], info["domain"]) == (rc.N_VARS, rc.N_INPUTS, rc.N_CONSTRAINTS, rc.DOMAIN)
    mats = gpu.reveal_cs_matrices()
    assert info["nnz"] == [len(m[1]) for m in mats] == [sum(len(r) for r in M) for M in rc.matrices()]
    for (ptr, col, val), M in zip(mats, rc.matrices()):
        assert gr.from_csr(ptr, col, val) == M


def test_the_circuit_holds_a_key_of_the_layouts_shape(circuit):
    k = circuit.key
    assert (k.n_vars, k.n_inputs, k.n_constraints, k.domain) == (rc.N_VARS, rc.N_INPUTS, rc.N_CONSTRAINTS, rc.DOMAIN)


@pytest.mark.parametrize("m", [1, 3, 65, 129])
def test_witness_parity(gpu, circuit, m):
    """batch 1, 3, 65 (past one wave), 129 (past UZK_G16_GROUP) under a random secret"""
    check_batch(gpu, circuit, SK, batch_points(m))


@pytest.mark.parametrize("name", list(EDGE_SKS))
def test_witness_parity_at_the_edge_scalars(gpu, circuit, name):
    """sk = 0, 1, l - 1 and a scalar whose low 128 bits are all set, each over the edge points and past a wave boundary"""
    check_batch(gpu, circuit, EDGE_SKS[name], batch_points(66))


_high = random.Random("gpu-reveal-cs-high")
ONES = (1 << 256) - 1
HIGH_SKS = {"2^256-1": ONES, "2^255": 1 << 255, "2^251": 1 << 251, "l": ed.L, "l+1": ed.L + 1, "2^32": 1 << 32, "2^224|2^31": 1 << 224 | 1 << 31,
            "random-with-bit-255": 1 << 255 | _high.getrandbits(255)}


@pytest.mark.parametrize("name", list(HIGH_SKS))
def test_witness_parity_under_secrets_up_to_256_bits(gpu, circuit, name):
    """sk is 256 plain bits and the circuit constrains only the bits, so every integer below 2^256 is a secret: all bits set; bit 255
    alone (255 neutral iterations, then one point); bit 251, the first above every secret below L; L and L + 1 (a multiple of every
    subgroup point's order, and one more); bit 32 alone and bit 224 with bit 31, where a word boundary decides the highest set bit
    below an iteration; a random secret with bit 255 set.  Each over the edge points and past a wave boundary; the reveal and the
    key are the integer multiples on the whole curve (a point with a component of order 8 among them).
    uzk_cp_reveal_prove_batch does not refuse a secret of L or more, but its contract is one below L (its response is computed mod L),
    so it is held against the statements only for the two secrets below L."""
    sk = HIGH_SKS[name]
    assert 0 <= sk < 1 << 256 and (sk < ed.L) == (name in ("2^32", "2^224|2^31"))
    check_batch(gpu, circuit, sk, batch_points(66), cross=sk < ed.L)


def test_the_witness_does_not_depend_on_the_batch(gpu, circuit):
    pts = batch_points(65)
    a = circuit.witness(SK, pts)
    b = circuit.witness(SK, pts[64:65])
    try:
        assert np.array_equal(a.download()[64], b.download()[0])
    finally:
        a.release(); b.release()


def _blinds(m, tag):
    rng = random.Random(f"reveal-cs-blinds-{tag}")
    return [rng.randrange(gr.R) for _ in range(m)], [rng.randrange(gr.R) for _ in range(m)]


def _blob_proof(blob):
    w = vr.parse_blob(blob)
    return (w[0], w[1]), ((w[3], w[2]), (w[5], w[4])), (w[6], w[7])


@pytest.mark.parametrize("m", [1, 3])
def test_proofs_verify_under_the_reference_key(gpu, circuit, vk, m):
    """uzk_reveal_prove_snark_batch -> uzk_g16_verify_batch under the verifying key parsed from the fixture head; one of them through
    the Python-integer verifier too; a batch with one statement altered is rejected"""
    pts = batch_points(m)
    r, s = _blinds(m, m)
    statements, blobs = circuit.prove(SK, pts, r, s)
    assert [list(st) for st in statements] == [[int(v) for v in oc.fr_to_ints(ref_witness(SK, p)[1:7])] for p in pts]
    assert _verify(vk, blobs, statements, m) == (True, [0] * m)
    assert gr.verify(vr.real_vk(), [1] + list(statements[m - 1]), _blob_proof(blobs[m - 1]))
    bent = [list(st) for st in statements]
    bent[m - 1][2] = (bent[m - 1][2] + 1) % Q
    assert _verify(vk, blobs, bent, m) == (False, [0] * m)


def test_a_proof_under_the_secret_of_all_ones_verifies(gpu, circuit, vk):
    """sk = 2^256 - 1, far above L: the R1CS constrains the 256 bits and nothing else, so the proof is one of the statement
    ([sk] e1, [sk] G) and is accepted under the reference's verifying key, on the device and by the Python-integer verifier; with one
    statement word altered it is rejected.  The two cards are the generator and a point with a component of order 8."""
    pts = batch_points(2)
    assert pts == [ed.G, ORDER8]
    r, s = _blinds(2, "ones")
    statements, blobs = circuit.prove(ONES, pts, r, s)
    assert [tuple(st) for st in statements] == [tuple(p) + tuple(ref_mul(ONES, p)) + tuple(ref_mul(ONES, ed.G)) for p in pts]
    assert [list(st) for st in statements] == [[int(v) for v in oc.fr_to_ints(ref_witness(ONES, p)[1:7])] for p in pts]
    assert _verify(vk, blobs, statements, "ones") == (True, [0, 0])
    assert gr.verify(vr.real_vk(), [1] + list(statements[1]), _blob_proof(blobs[1]))
    for word in (2, 5):                                      # reveal.x of the second card; then pk.y
        bent = [list(st) for st in statements]
        bent[1][word] = (bent[1][word] + 1) % Q
        assert _verify(vk, blobs, bent, "ones") == (False, [0, 0])


def test_the_device_path_equals_the_host_path_over_the_exported_matrices(gpu, circuit):
    """uzk_g16_prove_batch over a key made from uzk_reveal_cs_matrices and the restatement's z equals uzk_reveal_prove_snark_batch for
    the same r and s"""
    from uzkge_amd import reveal as rv
    pts = batch_points(2)
    r, s = _blinds(2, "host")
    rw, sw = oc.fr_from_ints(r).reshape(-1, 4), oc.fr_from_ints(s).reshape(-1, 4)
    _, dev = circuit.prove_snark_batch(rv.scalars_to_wire([SK])[0], rv.points_to_wire(pts), rw, sw)
    key = gr.load_real_key()
    args = gr.key_arrays(key, rc.N_VARS, rc.N_INPUTS, rc.N_CONSTRAINTS, rc.matrices())
    args["matrices"] = gpu.reveal_cs_matrices()
    with gpu.Groth16Key.from_arrays(**args) as host_key:
        z = np.stack([ref_witness(SK, p) for p in pts])
        assert np.array_equal(host_key.prove(z, rw, sw), dev)


def test_reveal_with_snark_is_the_plain_reveal_with_a_snark(gpu, circuit, vk):
    from uzkge_amd import reveal as rv
    cards = [(p, ed.add(p, ed.G)) for p in batch_points(2)]
    r, s = _blinds(2, "api")
    reveals, proofs, pk = rv.reveal_with_snark(SK, cards, circuit, r, s)
    want, _, want_pk = rv.reveal(SK, cards, [11, 12])
    assert reveals == want == [ed.mul(SK, c[0]) for c in cards] and pk == want_pk
    assert _verify(vk, proofs, [list(c[0]) + list(rvl) + list(pk) for c, rvl in zip(cards, reveals)], "api") == (True, [0, 0])


def test_refusals(gpu, circuit):
    from uzkge_amd import _native as N, reveal as rv
    from uzkge_amd.errors import UzkgeError
    lib = N.lib
    sk = rv.scalars_to_wire([SK])[0]
    good = rv.points_to_wire([POOL[0], POOL[1]])
    d_z = gpu.dev_alloc(32 * rc.N_VARS * 2)
    st = np.zeros((2, 6, 4), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call = lambda h, e1, m: lib.uzk_reveal_witness_batch(h, p(sk), p(e1), m, ctypes.c_void_p(d_z), p(st))
    try:
        assert call(circuit.handle, good, 2) == N.UZK_OK
        off = rv.points_to_wire([POOL[0], (POOL[1][0], (POOL[1][1] + 1) % Q)])
        assert not ed.on_curve(rv.points_from_wire(off)[1])
        assert call(circuit.handle, off, 2) == N.UZK_ERR_PARAMETER                      # e1 off the curve
        big = good.copy()
        big[1, 4:8] = ed.raw_wire([Q])[0]                                               # a coordinate >= q
        assert call(circuit.handle, big, 2) == N.UZK_ERR_PARAMETER
        assert call(circuit.handle, good, 0) == N.UZK_ERR_PARAMETER                      # m = 0
        assert call(circuit.handle, good, N.REVEAL_CS_MAX_BATCH + 1) == N.UZK_ERR_PARAMETER
        assert call(12345, good, 2) == N.UZK_ERR_PARAMETER and call(circuit.key.handle, good, 2) == N.UZK_ERR_PARAMETER
        r = np.zeros((2, 4), dtype=np.uint64)
        out = np.zeros((2, 32), dtype=np.uint64)
        assert lib.uzk_reveal_prove_snark_batch(circuit.handle, p(sk), p(off), p(r), p(r), 2, p(st), p(out)) == N.UZK_ERR_PARAMETER
        assert lib.uzk_reveal_prove_snark_batch(circuit.handle, p(sk), p(good), p(r), p(r), 0, p(st), p(out)) == N.UZK_ERR_PARAMETER
    finally:
        gpu.dev_free(d_z)
    # a key of another shape at create: one point short in a_query (so n_vars = 4868), in l_query, in h_query; another n_inputs
    key = gr.load_real_key()
    a = gr.key_arrays(key, rc.N_VARS, rc.N_INPUTS, rc.N_CONSTRAINTS, [])
    base = [a[f] for f in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "a_query", "b_g1_query", "l_query", "h_query", "b_g2_query")]
    for idx in (5, 7, 8):
        args = list(base)
        args[idx] = args[idx][:-1]
        with pytest.raises(UzkgeError):
            gpu.RevealCircuit(*args)
    with pytest.raises(UzkgeError):
        gpu.RevealCircuit(*base, n_inputs=6)
    # a released handle
    c2 = gpu.RevealCircuit(*base)
    h, inner = c2.handle, c2.key.handle
    c2.release()
    assert call(h, good, 2) == N.UZK_ERR_PARAMETER
    k = ctypes.c_uint64(0)
    assert lib.uzk_reveal_circuit_key(h, ctypes.byref(k)) == N.UZK_ERR_PARAMETER and lib.uzk_reveal_circuit_release(h) == N.UZK_ERR_PARAMETER
    assert lib.uzk_g16_key_info(inner, None, None, None, None, None) == N.UZK_ERR_PARAMETER      # the inner key went with the circuit
