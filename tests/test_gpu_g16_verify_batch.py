"""GPU: uzk_g16_verify_batch -- the Groth16 fold run to its verdict on the device -- against tests/g16_verify_ref.py's simulator and
restatement: the reference's golden reveal proof under its real key, batches of simulated proofs of a trapdoor key, every status
rule, and the fold's own outputs unchanged around it."""
import random

import numpy as np
import pytest

import g16_verify_ref as vr

pytestmark = pytest.mark.gpu
R, P = vr.R, vr.P
POOL = 65


def _key(gpu, key):
    return gpu.Groth16VerifierKey(*vr.key_wire(key))


def _weights(m, seed):
    rng = random.Random(f"g16-verify-batch-weights-{seed}")
    return [rng.randrange(1, 1 << 128) for _ in range(m)]


def _verify(dk, blobs, publics, weights):
    w = None if weights is None else vr.weights_wire(weights) if len(weights) else np.zeros((0, 4), dtype=np.uint64)
    accepted, status = dk.verify_batch(b"".join(blobs), vr.publics_wire(publics, dk.n_inputs), w)
    return accepted, [int(s) for s in status]


def _fold(dk, blobs, publics, weights):
    w = None if weights is None else vr.weights_wire(weights)
    return dk.fold(b"".join(blobs), vr.publics_wire(publics, dk.n_inputs), w)


@pytest.fixture(scope="module")
def trap7(gpu):
    """the l = 7 trapdoor key on the device and a pool of simulated proofs -- made once, never changed"""
    key, trap = vr.trapdoor_vk(7, "verify-batch")
    logs = vr.simulated_logs(trap, POOL, "verify-batch")
    proofs = [vr.proof_of_logs(e) for e in logs]
    dk = _key(gpu, key)
    yield dict(key=key, trap=trap, publics=[e[3] for e in logs], proofs=proofs, blobs=[vr.make_blob(p) for p in proofs], dk=dk)
    dk.release()


def test_the_golden_reveal_proof_under_the_real_key(gpu):
    key = vr.real_vk()
    public, proof = vr.golden()
    dk = _key(gpu, key)
    try:
        blob = vr.make_blob(proof)
        assert _verify(dk, [blob], [public], None) == (True, [0])
        bent = list(public)
        bent[2] = (bent[2] + 1) % R
        assert _verify(dk, [blob], [bent], None) == (False, [0])
        assert _verify(dk, [blob] * 2, [public, bent], _weights(2, 0)) == (False, [0, 0])
        assert _verify(dk, [blob] * 3, [public] * 3, _weights(3, 1)) == (True, [0, 0, 0])
    finally:
        dk.release()


def test_eight_proofs_and_three_ways_to_spoil_them(gpu, trap7):
    t = trap7
    blobs, pubs, w = t["blobs"][:8], t["publics"][:8], _weights(8, 2)
    before = _fold(t["dk"], blobs, pubs, w)
    assert _verify(t["dk"], blobs, pubs, w) == (True, [0] * 8)
    after = _fold(t["dk"], blobs, pubs, w)                              # uzk_g16_verify_fold around it: identical bytes
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert vr.accepts(t["key"], vr.fold(t["key"], blobs, pubs, w))
    bent = [list(r) for r in pubs]
    bent[5][3] = (bent[5][3] + 1) % R
    assert _verify(t["dk"], blobs, bent, w) == (False, [0] * 8)
    a, b, c = t["proofs"][3]
    other = list(blobs)
    other[3] = vr.make_blob((a, b, t["proofs"][4][2]))                  # C replaced by another curve point
    assert _verify(t["dk"], other, pubs, w) == (False, [0] * 8)
    assert not vr.accepts(t["key"], vr.fold(t["key"], other, pubs, w))
    k = t["key"]
    swapped = gpu.Groth16VerifierKey(*vr.key_wire(type(k)(alpha_g1=k.alpha_g1, beta_g2=k.gamma_g2, gamma_g2=k.beta_g2, delta_g2=k.delta_g2,
                                                             gamma_abc_g1=k.gamma_abc_g1)))
    try:
        assert _verify(swapped, blobs, pubs, w) == (False, [0] * 8)     # beta swapped with gamma
    finally:
        swapped.release()


@pytest.mark.parametrize("m", [0, 1, 52, 64, 65])
def test_batch_sizes(gpu, trap7, m):
    t = trap7
    w = _weights(m, m) if m != 1 else None
    assert _verify(t["dk"], t["blobs"][:m], t["publics"][:m], w) == (True, [0] * m)
    if m >= 1:
        bent = [list(r) for r in t["publics"][:m]]
        bent[m - 1][0] = (bent[m - 1][0] + 1) % R
        assert _verify(t["dk"], t["blobs"][:m], bent, w) == (False, [0] * m)


def test_every_status_among_good_proofs(gpu, trap7):
    """a proof with a nonzero status makes the verdict 0, its status byte says why, and the bytes are the fold's"""
    t = trap7
    crafted = vr.crafted(t["trap"], "verify-batch")
    blobs = t["blobs"][:2] + [c[1] for c in crafted] + t["blobs"][2:4]
    pubs = t["publics"][:2] + [c[2] for c in crafted] + t["publics"][2:4]
    w = _weights(len(blobs), 3)
    want = [0, 0] + [c[3] for c in crafted] + [0, 0]
    accepted, status = _verify(t["dk"], blobs, pubs, w)
    assert status == want and accepted is False
    assert [int(s) for s in _fold(t["dk"], blobs, pubs, w)[5]] == want
    for name, blob, pub, st in crafted:
        accepted, status = _verify(t["dk"], [t["blobs"][0], blob], [t["publics"][0], pub], _weights(2, 4))
        assert status == [0, st], name
        f = vr.fold(t["key"], [t["blobs"][0], blob], [t["publics"][0], pub], _weights(2, 4))
        assert accepted == (st == 0 and vr.accepts(t["key"], f)), name


def test_verdict_and_status_equal_the_restatement(gpu, trap7):
    t = trap7
    rng = random.Random("verify-batch-mixed")
    for case in range(3):
        idx = [rng.randrange(POOL) for _ in range(5)]
        blobs, pubs = [t["blobs"][i] for i in idx], [list(t["publics"][i]) for i in idx]
        if case == 1:
            pubs[rng.randrange(5)][rng.randrange(6)] = rng.randrange(R)
        if case == 2:
            blobs[0], pubs[0] = blobs[1], pubs[1]                       # a repeated proof is still a valid one
        w = _weights(5, 10 + case)
        f = vr.fold(t["key"], blobs, pubs, w)
        assert _verify(t["dk"], blobs, pubs, w) == (all(s == 0 for s in f["status"]) and vr.accepts(t["key"], f), f["status"])


def test_python_mirror_and_a_bad_key_point(gpu, trap7):
    from uzkge_amd import UzkgeError
    from uzkge_amd.poly_commit import Groth16VerifierKey, g16_proof_blob
    t, k = trap7, trap7["key"]
    mk = Groth16VerifierKey(k.alpha_g1, k.beta_g2, k.gamma_g2, k.delta_g2, k.gamma_abc_g1)
    try:
        blobs = [g16_proof_blob(*p) for p in t["proofs"][:3]]
        accepted, status = mk.verify_batch(blobs, t["publics"][:3], _weights(3, 20))
        assert accepted is True and list(status) == [0, 0, 0]
        accepted, status = mk.verify_batch(blobs, [t["publics"][0]] * 3, _weights(3, 20))
        assert accepted is False and list(status) == [0, 0, 0]
        accepted, status = mk.verify_batch([], [])
        assert accepted is True and len(status) == 0                    # the empty product
        with pytest.raises(UzkgeError):
            mk.verify_batch(blobs, t["publics"][:3])                    # a batch without weights
        mk.key.gamma_g2 = mk.key.gamma_g2.copy()
        mk.key.gamma_g2[8] ^= np.uint64(1)                              # gamma off the twist
        with pytest.raises(UzkgeError) as e:
            mk.verify_batch(blobs, t["publics"][:3], _weights(3, 20))
        assert e.value.kind == "ParameterError" and "g2[1]" in str(e.value)
    finally:
        mk.release()
