"""CPU: the batch form of the Groth16 verifier (tests/g16_verify_ref.py) pinned on the reference's golden reveal proof and on simulated
proofs of trapdoor keys, and the argument checks of uzk_g16_vk_create / uzk_g16_vk_release / uzk_g16_vk_info / uzk_g16_verify_fold,
which answer before anything touches a device."""
import ctypes
import random

import numpy as np
import pytest

import g16_ref as gr
import g16_verify_ref as vr

R, P = vr.R, vr.P


def test_the_fixture_is_the_committed_one():
    assert vr.sha256_of(vr.GOLDEN_JSON) == vr.GOLDEN_SHA256
    assert gr.sha256_of(gr.HEAD) == gr.HEAD_SHA256
    signals, proof = vr.golden()
    assert len(signals) == 6 and all(0 <= v < R for v in signals) and all(p is not None for p in proof)
    assert len(vr.real_vk().gamma_abc_g1) == 7


def test_the_golden_reveal_proof_under_the_reference_key():
    """accepted as it is, rejected with the first public signal incremented; the blob round-trips"""
    key = vr.real_vk()
    signals, proof = vr.golden()
    assert gr.verify(key, [1] + signals, proof)
    assert not gr.verify(key, [1, (signals[0] + 1) % R] + signals[1:], proof)
    blob = vr.make_blob(proof)
    assert len(blob) == vr.PROOF_BYTES and vr.points_of_words(vr.parse_blob(blob)) == proof and vr.status_of(blob) == vr.OK
    f = vr.fold(key, [blob], [signals])
    assert f["a"] == [proof[0]] and f["b"] == [proof[1]] and f["alpha"] == key.alpha_g1 and f["c"] == proof[2]
    assert f["x"] == vr.x_of(key, signals) and vr.accepts(key, f)


@pytest.mark.parametrize("l", [1, 7])
def test_simulated_proofs_verify(l):
    key, trap = vr.trapdoor_vk(l, "host")
    proofs, publics = vr.simulated_batch(trap, 2, f"host-{l}")
    for proof, pub in zip(proofs, publics):
        assert gr.verify(key, [1] + pub, proof)
    if l > 1:
        bad = [(publics[0][0] + 1) % R] + publics[0][1:]
        assert not gr.verify(key, [1] + bad, proofs[0])
    else:
        assert not gr.verify(key, [1], (proofs[0][0], proofs[0][1], proofs[1][2]))


def test_the_folded_equation_under_random_weights():
    key, trap = vr.trapdoor_vk(7, "fold")
    proofs, publics = vr.simulated_batch(trap, 3, "fold")
    rng = random.Random("g16-verify-host-weights")
    weights = [rng.getrandbits(128) | 1 for _ in range(3)]
    blobs = [vr.make_blob(p) for p in proofs]
    f = vr.fold(key, blobs, publics, weights)
    assert f["status"] == [0, 0, 0] and vr.accepts(key, f)
    bad = [list(row) for row in publics]
    bad[1][3] = (bad[1][3] + 1) % R                                 # one invalid proof: its public input changed
    f = vr.fold(key, blobs, bad, weights)
    assert f["status"] == [0, 0, 0] and not vr.accepts(key, f)
    swapped = [blobs[0], vr.make_blob((proofs[1][0], proofs[1][1], proofs[2][2])), blobs[2]]       # ... or its C
    assert not vr.accepts(key, vr.fold(key, swapped, publics, weights))


def test_the_closed_form_of_a_fold_agrees_with_the_group_law():
    key, trap = vr.trapdoor_vk(7, "logs")
    logs = vr.simulated_logs(trap, 3, "logs")
    weights = [(1 << 128) - 1, 1, R - 1]
    f = vr.fold(key, [vr.make_blob(vr.proof_of_logs(e)) for e in logs], [e[3] for e in logs], weights)
    want = vr.fold_logs(trap, logs, weights)
    g = gr._g1_fixed()
    assert f["a"] == [g(v) for v in want["a_log"]] and (f["alpha"], f["x"], f["c"]) == (want["alpha"], want["x"], want["c"])
    assert vr.accepts(key, f)


def test_the_status_rules_on_crafted_blobs():
    key, trap = vr.trapdoor_vk(3, "status")
    cases = vr.crafted(trap)
    assert {st for _, _, _, st in cases} == {0, 1, 2, 3}
    for name, blob, _, expected in cases:
        assert vr.status_of(blob) == expected, name
    # a bad proof contributes nothing: the fold over (good, bad, good) is the fold over the good ones
    proofs, publics = vr.simulated_batch(trap, 2, "status")
    blobs = [vr.make_blob(p) for p in proofs]
    name, bad, bad_pub, st = next(c for c in cases if c[3] == 3)
    full = vr.fold(key, [blobs[0], bad, blobs[1]], [publics[0], bad_pub, publics[1]], [5, 7, 11])
    part = vr.fold(key, blobs, publics, [5, 11])
    assert full["status"] == [0, 3, 0] and full["a"][1] is None and full["b"][1] is None
    assert (full["alpha"], full["x"], full["c"]) == (part["alpha"], part["x"], part["c"]) and vr.accepts(key, full)
    # infinity is all zeros and well-formed
    assert vr.status_of(bytes(256)) == 0


def test_entry_points_check_their_arguments_before_the_device():
    """Exported, declared, and refusing null pointers, a wrong number of inputs, a batch above the cap, an unweighted batch and unknown
    or released handles as ParameterError with or without a GPU; without one a well-formed uzk_g16_vk_create is a DeviceError."""
    from uzkge_amd import UzkgeError, _native as N, backend as b
    for name in ("uzk_g16_vk_create", "uzk_g16_vk_release", "uzk_g16_vk_info", "uzk_g16_verify_fold"):
        assert name in N.PROTOTYPES and hasattr(N.lib, name)
    assert (N.G16_VERIFY_MAX_BATCH, N.G16_VERIFY_MAX_INPUTS, N.G16_PROOF_BYTES) == (4096, 1024, 256)
    assert ctypes.sizeof(N.G16VkDesc) == 8 + 64 + 3 * 128 + 8
    h = ctypes.c_uint64(0)
    z = np.zeros(4096, dtype=np.uint64)
    p = z.ctypes.data_as(ctypes.c_void_p)
    fold, create = N.lib.uzk_g16_verify_fold, N.lib.uzk_g16_vk_create
    assert create(None, ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    d = N.G16VkDesc()
    d.n_inputs, d.gamma_abc_g1 = 1, z.ctypes.data
    assert create(ctypes.byref(d), None) == N.UZK_ERR_PARAMETER
    d.n_inputs = 0                                                   # not even the constant one
    assert create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    d.n_inputs = N.G16_VERIFY_MAX_INPUTS + 1
    assert create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    d.n_inputs, d.gamma_abc_g1 = 7, None                             # inputs without their points
    assert create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    assert b"gamma_abc_g1" in N.lib.uzk_last_error()
    for bad in (0, 12345, (6 << 59) | 99, (5 << 59) | 1):            # unknown handles (the last: a PlonK key's tag)
        assert N.lib.uzk_g16_vk_release(bad) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_g16_vk_info(bad, None, None) == N.UZK_ERR_PARAMETER
        assert fold(bad, p, p, 1, None, p, p, p, p, p, p) == N.UZK_ERR_PARAMETER
        assert fold(bad, p, p, 2, p, p, p, p, p, p, p) == N.UZK_ERR_PARAMETER
        assert fold(bad, p, p, 0, None, p, p, p, p, p, p) == N.UZK_ERR_PARAMETER
    assert fold(12345, p, p, N.G16_VERIFY_MAX_BATCH + 1, p, p, p, p, p, p, p) == N.UZK_ERR_PARAMETER
    assert b"4097" in N.lib.uzk_last_error()
    assert fold(12345, p, p, 2, None, p, p, p, p, p, p) == N.UZK_ERR_PARAMETER        # unweighted sums let errors cancel
    assert b"weight" in N.lib.uzk_last_error()
    for hole in range(5, 11):                                        # a_out .. status_out
        args = [12345, p, p, 1, None, p, p, p, p, p, p]
        args[hole] = None
        assert fold(*args) == N.UZK_ERR_PARAMETER
        assert b"null pointer" in N.lib.uzk_last_error()
    assert fold(12345, None, p, 1, None, p, p, p, p, p, p) == N.UZK_ERR_PARAMETER
    if b.device_count() == 0:
        from uzkge_amd.poly_commit import Groth16VerifierKey
        with pytest.raises(UzkgeError) as e:
            Groth16VerifierKey.from_key_bytes(open(gr.HEAD, "rb").read()[:vr.VK_BYTES])
        assert e.value.kind == "DeviceError"


def test_the_key_parser_of_the_binding_agrees_with_the_restatement():
    from uzkge_amd.poly_commit import Groth16VerifierKey, g16_proof_blob
    key = vr.real_vk()
    alpha, beta, gamma, delta, ic = Groth16VerifierKey.parse_key_bytes(open(gr.HEAD, "rb").read())
    assert (alpha, beta, gamma, delta, ic) == (key.alpha_g1, key.beta_g2, key.gamma_g2, key.delta_g2, key.gamma_abc_g1)
    _, proof = vr.golden()
    assert g16_proof_blob(*proof) == vr.make_blob(proof) and g16_proof_blob(None, None, None) == bytes(256)
