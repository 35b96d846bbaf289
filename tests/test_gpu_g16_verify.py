"""GPU: uzk_g16_vk_create / uzk_g16_verify_fold against tests/g16_verify_ref.py, bit-exact on canonical words: the reference's golden
reveal proof under the reference's key, folds of simulated proofs of trapdoor keys through to the pairing product, the sizes at the
kernels' edges, scalar and point edge cases, cancellation, every status at three positions, and the life of a key."""
import ctypes
import random

import numpy as np
import pytest

import g16_ref as gr
import g16_verify_ref as vr
import g2_ref as g2

pytestmark = pytest.mark.gpu
R, P = vr.R, vr.P
POOL = 16


def _key(gpu, key):
    return gpu.Groth16VerifierKey(*vr.key_wire(key))


def _run(dk, blobs, publics, weights):
    l = dk.n_inputs
    w = None if weights is None else vr.weights_wire(weights) if len(weights) else np.zeros((0, 4), dtype=np.uint64)
    return dk.fold(b"".join(blobs), vr.publics_wire(publics, l), w)


def _points(gpu, got):
    """the device's outputs as integer points: (a list, b list, alpha, x, c)"""
    a, b, alpha, x, c, _ = got
    return gr.g1_from_wire(a) if len(a) else [], [g2.point_from_wire(row) for row in b], vr.jac_point(alpha), vr.jac_point(x), vr.jac_point(c)


def _same(gpu, first, second):
    """two results of one fold: a, b and the status bit for bit, the three sums as group elements (a Jacobian point has many forms)"""
    for k in (0, 1, 5):
        assert np.array_equal(first[k], second[k])
    assert _points(gpu, first)[2:] == _points(gpu, second)[2:]


def _check(gpu, key, got, blobs, publics, weights):
    """every output equals the restatement's; returns the restatement"""
    want = vr.fold(key, blobs, publics, weights)
    a, b, _, _, _, status = got
    assert list(status) == want["status"]
    assert np.array_equal(a, vr.a_wire(want["a"])) and np.array_equal(b, vr.b_wire(want["b"]))
    _, _, alpha, x, c = _points(gpu, got)
    assert (alpha, x, c) == (want["alpha"], want["x"], want["c"])
    return want


@pytest.fixture(scope="module")
def trap7(gpu):
    """the l = 7 trapdoor key on the device, a pool of simulated proofs as logarithms, points and blobs -- made once, never changed"""
    key, trap = vr.trapdoor_vk(7, "gpu")
    logs = vr.simulated_logs(trap, POOL, "gpu")
    proofs = [vr.proof_of_logs(e) for e in logs]
    dk = _key(gpu, key)
    yield dict(key=key, trap=trap, logs=logs, proofs=proofs, blobs=[vr.make_blob(p) for p in proofs], dk=dk)
    dk.release()


def test_the_golden_proof_under_the_real_key(gpu):
    key = vr.real_vk()
    signals, proof = vr.golden()
    from uzkge_amd.poly_commit import Groth16VerifierKey, g16_proof_blob
    dk = Groth16VerifierKey.from_key_bytes(open(gr.HEAD, "rb").read()[:vr.VK_BYTES])
    try:
        assert dk.info() == (7, 0)
        got = dk.fold([g16_proof_blob(*proof)], [signals])
        a, b, alpha, x, c = _points(gpu, got)
        assert list(got[5]) == [0]
        assert a == [proof[0]] and b == [proof[1]] and alpha == key.alpha_g1 and c == proof[2]
        assert x == vr.x_of(key, signals)
        assert np.array_equal(got[0], gr.g1_to_wire([proof[0]])) and np.array_equal(got[1], g2.points_to_wire([proof[1]]))
        assert vr.product_is_one(key, a, b, alpha, x, c)
        bad = dk.fold([g16_proof_blob(*proof)], [[(signals[0] + 1) % R] + signals[1:]])
        assert list(bad[5]) == [0] and not vr.product_is_one(key, *_points(gpu, bad))
    finally:
        dk.release()


def test_the_fold_identity(gpu, trap7):
    """m = 8, 128-bit weights: every output matches the restatement, the product of 11 Miller loops is one; with one public input
    changed every status is still 0 and the product is not one"""
    rng = random.Random("g16-verify-gpu-fold")
    m = 8
    weights = [rng.getrandbits(128) for _ in range(m)]
    blobs, publics = trap7["blobs"][:m], [e[3] for e in trap7["logs"][:m]]
    got = _run(trap7["dk"], blobs, publics, weights)
    _check(gpu, trap7["key"], got, blobs, publics, weights)
    a, b, alpha, x, c = _points(gpu, got)
    assert len(a) + 3 == 11 and vr.product_is_one(trap7["key"], a, b, alpha, x, c)
    bad = [list(row) for row in publics]
    bad[5][2] = (bad[5][2] + 1) % R
    got = _run(trap7["dk"], blobs, bad, weights)
    _check(gpu, trap7["key"], got, blobs, bad, weights)
    assert not any(got[5]) and not vr.product_is_one(trap7["key"], *_points(gpu, got))


def _cycled(trap7, m, seed):
    rng = random.Random(f"g16-verify-gpu-size-{seed}")
    idx = [i % POOL for i in range(m)]
    return idx, [rng.getrandbits(128) for _ in range(m)]


@pytest.mark.parametrize("m", [0, 1, 2, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_at_the_kernels_edges(gpu, trap7, m):
    """the pool's proofs cycled under fresh weights; expected values in closed form from the logarithms (g16_verify_ref.fold_logs,
    which tests/test_g16_verify_ref_host.py holds to the group-law restatement)"""
    idx, weights = _cycled(trap7, m, m)
    entries = [trap7["logs"][i] for i in idx]
    got = _run(trap7["dk"], [trap7["blobs"][i] for i in idx], [e[3] for e in entries], weights if m != 1 else None)
    if m == 1:
        weights = [1]
    want = vr.fold_logs(trap7["trap"], entries, weights)
    a, b, alpha, x, c = _points(gpu, got)
    assert len(got[5]) == m and not any(got[5])
    g = gr._g1_fixed()
    assert a == [g(v) for v in want["a_log"]] and b == [trap7["proofs"][i][1] for i in idx]
    assert np.array_equal(got[1], g2.points_to_wire([trap7["proofs"][i][1] for i in idx]) if m else np.zeros((0, 16), dtype=np.uint64))
    if m == 0:
        assert (alpha, x, c) == (None, None, None)
    else:
        assert (alpha, x, c) == (want["alpha"], want["x"], want["c"])


def test_the_largest_batch_and_one_more(gpu, trap7):
    from uzkge_amd import UzkgeError
    m = 4096
    idx, weights = _cycled(trap7, m, "max")
    entries = [trap7["logs"][i] for i in idx]
    blobs = [trap7["blobs"][i] for i in idx]
    got = _run(trap7["dk"], blobs, [e[3] for e in entries], weights)
    want = vr.fold_logs(trap7["trap"], entries, weights)
    assert len(got[5]) == m and not got[5].any()
    _, _, alpha, x, c = _points(gpu, got)
    assert (alpha, x, c) == (want["alpha"], want["x"], want["c"])
    g = gr._g1_fixed()
    for i in (0, 1, 63, 64, 2047, 2048, 4032, 4095):
        assert gr.g1_from_wire(got[0][i]) == [g(want["a_log"][i])]
        assert g2.point_from_wire(got[1][i]) == trap7["proofs"][idx[i]][1]
    with pytest.raises(UzkgeError) as e:
        _run(trap7["dk"], blobs + blobs[:1], [en[3] for en in entries] + [entries[0][3]], weights + [1])
    assert e.value.kind == "ParameterError"


@pytest.mark.parametrize("l", [1, 2, 33])
def test_numbers_of_inputs(gpu, l):
    key, trap = vr.trapdoor_vk(l, "gpu-l")
    proofs, publics = vr.simulated_batch(trap, 3, f"gpu-l-{l}")
    blobs = [vr.make_blob(p) for p in proofs]
    weights = [3, 1 << 127, R - 2]
    dk = _key(gpu, key)
    try:
        assert dk.info() == (l, 0)
        got = _run(dk, blobs, publics, weights)
        _check(gpu, key, got, blobs, publics, weights)
        assert vr.product_is_one(key, *_points(gpu, got))
    finally:
        dk.release()


def test_scalar_edges(gpu, trap7):
    """weights 0, 1, r - 1, 2^128 - 1; public inputs 0, 1, r - 1"""
    key, trap = trap7["key"], trap7["trap"]
    weights = [0, 1, R - 1, (1 << 128) - 1]
    publics = [[0] * 6, [1] * 6, [R - 1] * 6, [0, 1, R - 1, 1, 0, R - 1]]
    rng = random.Random("g16-verify-gpu-scalars")
    proofs = [vr.simulate(trap, rng.randrange(1, R), rng.randrange(1, R), pub) for pub in publics]
    blobs = [vr.make_blob(p) for p in proofs]
    got = _run(trap7["dk"], blobs, publics, weights)
    want = _check(gpu, key, got, blobs, publics, weights)
    assert want["a"][0] is None and not got[0][0].any() and got[1][0].any()          # weight 0: rho A = O, B as it is
    assert vr.product_is_one(key, *_points(gpu, got))


def test_points_at_infinity(gpu, trap7):
    """a gamma_abc_g1[j] at infinity; A, B or C at infinity (well-formed: status 0)"""
    key, trap = vr.trapdoor_vk(4, "gpu-inf", ic=[5, 0, 7, 0])
    assert key.gamma_abc_g1[1] is None and key.gamma_abc_g1[3] is None
    proofs, publics = vr.simulated_batch(trap, 2, "gpu-inf")
    blobs = [vr.make_blob(p) for p in proofs]
    dk = _key(gpu, key)
    try:
        got = _run(dk, blobs, publics, [11, 13])
        _check(gpu, key, got, blobs, publics, [11, 13])
        assert vr.product_is_one(key, *_points(gpu, got))
    finally:
        dk.release()
    A, B, C = trap7["proofs"][0]
    pub = trap7["logs"][0][3]
    blobs = [vr.make_blob(p) for p in ((None, B, C), (A, None, C), (A, B, None), (None, None, None), (A, B, C))]
    weights = [2, 3, 5, 7, 11]
    got = _run(trap7["dk"], blobs, [pub] * 5, weights)
    want = _check(gpu, trap7["key"], got, blobs, [pub] * 5, weights)
    assert want["status"] == [0] * 5 and want["a"][0] is None and want["b"][1] is None


def test_cancellation_and_doubling(gpu, trap7):
    """the same C under rho and r - rho: c_out at infinity (and alpha_out: the weights sum to zero); the same proof twice under equal
    weights: the additions of the MSM meet equal operands"""
    rho = (1 << 127) + 12345
    blobs, pub = [trap7["blobs"][3]] * 2, [trap7["logs"][3][3]] * 2
    got = _run(trap7["dk"], blobs, pub, [rho, R - rho])
    want = _check(gpu, trap7["key"], got, blobs, pub, [rho, R - rho])
    assert want["c"] is None and want["alpha"] is None and want["x"] is None
    assert not np.any(got[4][8:12]) and not np.any(got[2][8:12])                    # z = 0
    got = _run(trap7["dk"], blobs, pub, [rho, rho])
    _check(gpu, trap7["key"], got, blobs, pub, [rho, rho])
    assert vr.product_is_one(trap7["key"], *_points(gpu, got))
    blobs, pub = [trap7["blobs"][3]] * 4, [trap7["logs"][3][3]] * 4
    got = _run(trap7["dk"], blobs, pub, [1, 1, 1, 1])
    _check(gpu, trap7["key"], got, blobs, pub, [1, 1, 1, 1])


@pytest.fixture(scope="module")
def crafted7(trap7):
    return vr.crafted(trap7["trap"], seed=7)


@pytest.mark.parametrize("position", ["first", "middle", "last"])
def test_every_status_at_three_positions(gpu, trap7, crafted7, position):
    """each crafted blob among four good proofs: the sums are the fold of the good subset, a bad proof's a_out and b_out are zeros"""
    good_blobs, good_pub = trap7["blobs"][:4], [e[3] for e in trap7["logs"][:4]]
    at = dict(first=0, middle=2, last=4)[position]
    rng = random.Random(f"g16-verify-gpu-status-{position}")
    seen = set()
    for name, blob, pub, expected in crafted7:
        blobs, publics = list(good_blobs), list(good_pub)
        blobs.insert(at, blob); publics.insert(at, pub)
        weights = [rng.getrandbits(128) for _ in range(5)]
        got = _run(trap7["dk"], blobs, publics, weights)
        assert list(got[5]) == [expected if i == at else 0 for i in range(5)], name
        want = _check(gpu, trap7["key"], got, blobs, publics, weights)
        if expected != 0:
            assert not got[0][at].any() and not got[1][at].any(), name
            part = vr.fold(trap7["key"], good_blobs, good_pub, weights[:at] + weights[at + 1:])
            assert (want["alpha"], want["x"], want["c"]) == (part["alpha"], part["x"], part["c"]), name
        seen.add(expected)
    assert seen == {0, 1, 2, 3}


def test_a_second_context(gpu, trap7):
    """the key serves a fold from another context of its device; that context's workspaces die with it"""
    blobs, publics, weights = trap7["blobs"][:3], [e[3] for e in trap7["logs"][:3]], [7, 8, 9]
    first = _run(trap7["dk"], blobs, publics, weights)
    ctx = gpu.ctx_create_on(0)
    try:
        gpu.ctx_set_current(ctx)
        second = _run(trap7["dk"], blobs, publics, weights)
    finally:
        gpu.ctx_set_current(0)
        gpu.ctx_destroy(ctx)
    _same(gpu, first, second)
    _check(gpu, trap7["key"], second, blobs, publics, weights)


def test_repeated_calls_reuse_the_workspaces(gpu, trap7):
    """a large fold, a small one, the large one again: identical results (the workspaces grow once and are reused)"""
    idx, weights = _cycled(trap7, 300, "again")
    args = ([trap7["blobs"][i] for i in idx], [trap7["logs"][i][3] for i in idx], weights)
    big = _run(trap7["dk"], *args)
    small = _run(trap7["dk"], trap7["blobs"][:2], [e[3] for e in trap7["logs"][:2]], [1, 2])
    _check(gpu, trap7["key"], small, trap7["blobs"][:2], [e[3] for e in trap7["logs"][:2]], [1, 2])
    again = _run(trap7["dk"], *args)
    _same(gpu, big, again)
    want = vr.fold_logs(trap7["trap"], [trap7["logs"][i] for i in idx], weights)
    assert _points(gpu, again)[2:] == (want["alpha"], want["x"], want["c"])


def test_key_lifecycle(gpu, trap7):
    """two keys alive at once; release; use after release is an error; uzk_shutdown with a key left"""
    from uzkge_amd import UzkgeError, _native as N
    key1, trap1 = vr.trapdoor_vk(1, "gpu-life")
    proofs, publics = vr.simulated_batch(trap1, 1, "gpu-life")
    a, b = _key(gpu, key1), _key(gpu, trap7["key"])
    try:
        assert a.handle != b.handle != trap7["dk"].handle and (a.n_inputs, b.n_inputs) == (1, 7)
        for _ in range(2):
            got = _run(a, [vr.make_blob(proofs[0])], publics, None)
            _check(gpu, key1, got, [vr.make_blob(proofs[0])], publics, None)
            got = _run(b, trap7["blobs"][:1], [trap7["logs"][0][3]], None)
            _check(gpu, trap7["key"], got, trap7["blobs"][:1], [trap7["logs"][0][3]], None)
        handle = a.handle
        a.release()
        a.handle = handle
        with pytest.raises(UzkgeError) as e:
            _run(a, [vr.make_blob(proofs[0])], publics, None)
        assert e.value.kind == "ParameterError"
        a.handle = 0
        assert N.lib.uzk_g16_vk_info(handle, None, None) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_g16_vk_release(handle) == N.UZK_ERR_PARAMETER
        left, pool = b.handle, trap7["dk"].handle
        gpu.shutdown()                       # frees the keys that are left
        b.handle = 0
        assert N.lib.uzk_g16_vk_info(left, None, None) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_g16_vk_info(pool, None, None) == N.UZK_ERR_PARAMETER
    finally:
        gpu.init(0)
        a.release()
        b.release()
    trap7["dk"].handle = 0                   # gone with the shutdown: the module's key is made again
    trap7["dk"] = _key(gpu, trap7["key"])
    got = _run(trap7["dk"], trap7["blobs"][:2], [e[3] for e in trap7["logs"][:2]], [3, 4])
    _check(gpu, trap7["key"], got, trap7["blobs"][:2], [e[3] for e in trap7["logs"][:2]], [3, 4])
