"""CPU: the batch form of the verifier (tests/plonk_batch_ref.py) pinned on the reference's golden proofs, and the argument checks of
the verifier entry points (uzk_vk_create, uzk_vk_set_public_key, uzk_verify_fold), which run before anything touches a device."""
import copy
import ctypes

import numpy as np
import pytest

import bn254_py as opy
import plonk_batch_ref as br
import plonk_golden_verifier as gv

CASES = [(52, 16384), (20, 4096)]


@pytest.fixture(scope="module")
def g2():
    return br.load_g2()


def _verdict(vk, proof, pi, cards, g2):
    left, right = br.fold([br.terms(vk, proof, pi, br.prefix(cards))], [1])
    return br.accepts(left, right, g2)


@pytest.mark.parametrize("cards,cs_size", CASES)
def test_the_fold_of_one_proof_agrees_with_the_verifier(cards, cs_size, g2):
    """m = 1, weight 1: the pairing check on the flattened terms gives gv.verify's verdict -- accepting the golden proof, rejecting
    each tampering of tests/test_oracle_golden_proof.py."""
    vk, proof, pi = gv.load_golden(cards)
    assert gv.verify(vk, proof, pi, n_cards=cards, g2=g2) and _verdict(vk, proof, pi, cards, g2)
    p2 = copy.deepcopy(proof); p2["w"][3] = (p2["w"][3] + 1) % opy.R
    pi2 = list(pi); pi2[100] = (pi2[100] + 1) % opy.R
    p3 = copy.deepcopy(proof); p3["cm_t"][2] = opy.g1_add(p3["cm_t"][2], opy.G1_GEN)
    vk2 = copy.deepcopy(vk); vk2["cm_shuffle_public_key"][5] = opy.g1_add(vk2["cm_shuffle_public_key"][5], opy.G1_GEN)
    for v, p, x, c in ((vk, p2, pi, cards), (vk, proof, pi2, cards), (vk, p3, pi, cards), (vk2, proof, pi, cards), (vk, proof, pi, cards - 1)):
        assert not gv.verify(v, p, x, n_cards=c, g2=g2)
        assert not _verdict(v, p, x, c, g2)


def test_the_challenges_and_the_number_of_bases():
    """65 terms over 55 distinct bases on the right for the 52-card key (61 places, five of them hold the point at infinity and two of
    the key's commitments are equal), 2 bases on the left."""
    vk, proof, pi = gv.load_golden(52)
    left, right = br.terms(vk, proof, pi, br.prefix(52))
    assert len({b for b, _ in left}) == 2 and len({b for b, _ in right if b is not None}) == 55
    assert len(right) == 15 + 43 + 4 + 3 and sum(1 for b, _ in right if b is None) == 5
    ch = br.challenges(vk, proof, pi, br.prefix(52))
    assert len(set(ch)) == 7 and all(0 < c < opy.R for c in ch)


@pytest.mark.parametrize("cards,cs_size", CASES)
def test_a_batch_under_distinct_weights(cards, cs_size, g2):
    vk, proof, pi = gv.load_golden(cards)
    rng = np.random.default_rng(7)
    weights = [int.from_bytes(rng.bytes(16), "little") | 1 for _ in range(3)]
    assert len(set(weights)) == 3
    good = br.terms(vk, proof, pi, br.prefix(cards))
    left, right = br.fold([good, good, good], weights)
    assert br.accepts(left, right, g2)
    # three copies: both sides are (sum of the weights) times one proof's
    l1, r1 = br.fold([good], [1])
    total = sum(weights) % opy.R
    assert left == opy.g1_mul(l1, total) and right == opy.g1_mul(r1, total)
    bad = copy.deepcopy(proof); bad["z_omega"] = (bad["z_omega"] + 1) % opy.R
    left, right = br.fold([good, br.terms(vk, bad, pi, br.prefix(cards)), good], weights)
    assert not br.accepts(left, right, g2)


def test_verifier_entry_points_check_their_arguments_before_the_device():
    """Exported, declared, and refusing null pointers, unknown handles, a batch above the cap and an unweighted batch as
    ParameterError with or without a GPU; without one a well-formed uzk_vk_create is a DeviceError (no CPU fallback)."""
    from uzkge_amd import UzkgeError, _native as N, backend as b
    for name in ("uzk_vk_create", "uzk_vk_release", "uzk_vk_info", "uzk_vk_set_public_key", "uzk_verify_fold"):
        assert name in N.PROTOTYPES and hasattr(N.lib, name)
    assert "uzk_test_keccak256" in N.TEST_PROTOTYPES
    assert N.VERIFY_MAX_BATCH == 4096
    h = ctypes.c_uint64(0)
    z = np.zeros(4096, dtype=np.uint64)
    p = z.ctypes.data_as(ctypes.c_void_p)
    assert N.lib.uzk_vk_create(None, ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    d = N.VkDesc()
    assert N.lib.uzk_vk_create(ctypes.byref(d), None) == N.UZK_ERR_PARAMETER
    d.cs_size, d.n_pi = 4096, 1025                                   # more public inputs than the entry point takes
    assert N.lib.uzk_vk_create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    d.cs_size, d.n_pi = 4097, 0                                      # no domain of that size
    assert N.lib.uzk_vk_create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    d.cs_size, d.n_pi, d.transcript_prefix_len = 4096, 0, 257        # a longer prefix than the descriptor allows
    assert N.lib.uzk_vk_create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    d.transcript_prefix_len = 64                                     # ... and one without its bytes
    assert N.lib.uzk_vk_create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    d.transcript_prefix_len, d.n_pi = 0, 4                           # public inputs without the key's constants
    assert N.lib.uzk_vk_create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    for bad in (0, 12345, (1 << 62) | 3):                            # unknown handles
        assert N.lib.uzk_vk_release(bad) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_vk_info(bad, None, None, None, None) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_vk_set_public_key(bad, p) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_verify_fold(bad, p, p, 1, None, p, p, p, None) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_verify_fold(bad, p, p, 2, p, p, p, p, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_vk_set_public_key(12345, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_verify_fold(12345, p, p, N.VERIFY_MAX_BATCH + 1, p, p, p, p, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_verify_fold(12345, p, p, 2, None, p, p, p, None) == N.UZK_ERR_PARAMETER        # unweighted sums let errors cancel
    assert N.lib.uzk_verify_fold(12345, None, p, 1, None, p, p, p, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_verify_fold(12345, p, p, 1, None, None, p, p, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_verify_fold(12345, p, p, 1, None, p, p, None, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_test_keccak256(None, None, 1, None) == N.UZK_ERR_PARAMETER
    if b.device_count() == 0:
        vk, _, _ = gv.load_golden(20)
        from uzkge_amd.poly_commit import PlonkVerifierKey
        with pytest.raises(UzkgeError) as e:
            PlonkVerifierKey(vk, br.prefix(20))
        assert e.value.kind == "DeviceError"
        msg = np.zeros(8, dtype=np.uint8)
        off = np.array([0, 8], dtype=np.uint64)
        out = np.zeros(32, dtype=np.uint8)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert N.lib.uzk_test_keccak256(P(msg), P(off), 1, P(out)) == N.UZK_ERR_DEVICE
