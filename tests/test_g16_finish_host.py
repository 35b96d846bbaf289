"""CPU-side checks of the device finish of the Groth16 prover: the bindings declare the new entry points and the built library exports
them, and the blob encoding the device writes -- restated here in Python integers from a uzk_g16_proof -- takes the reference's own
golden reveal proof (tests/golden/groth16_reveal_golden.json) back into its own words."""
import json

import numpy as np

import bn254_py as opy
import g16_verify_ref as vr
import oracle_c as oc

NEW = ("uzk_msm_g2_batch_finish", "uzk_g16_prove_batch_finish", "uzk_reveal_prove_snark_batch_finish")
HOOK = "uzk_test_g16_finish"


def test_the_new_entry_points_are_declared_and_exported():
    from uzkge_amd import _native as N
    for name in NEW:
        assert name in N.PROTOTYPES and hasattr(N.lib, name), name
        assert getattr(N.lib, name).argtypes == N.PROTOTYPES[name][1], name
    assert HOOK in N.TEST_PROTOTYPES and HOOK not in N.PROTOTYPES and hasattr(N.lib, HOOK)
    assert len(N.PROTOTYPES["uzk_g16_prove_batch_finish"][1]) == 9 and len(N.PROTOTYPES["uzk_msm_g2_batch_finish"][1]) == 7
    assert len(N.PROTOTYPES["uzk_reveal_prove_snark_batch_finish"][1]) == 10 and len(N.TEST_PROTOTYPES[HOOK][1]) == 8


def test_the_null_output_refusals_need_no_device():
    """the argument checks come before the device is touched"""
    import ctypes
    from uzkge_amd import _native as N
    z = np.zeros((1, 4), dtype=np.uint64)
    p = z.ctypes.data_as(ctypes.c_void_p)
    assert N.lib.uzk_g16_prove_batch_finish(1, p, 0, p, p, 1, None, None, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_msm_g2_batch_finish(1, 0, p, 1, 1, None, None) == N.UZK_ERR_PARAMETER


def encode(proof_words_mont) -> bytes:
    """g16_encode restated: a uzk_g16_proof as 32 uint64 (a.x a.y | b.x.c0 b.x.c1 b.y.c0 b.y.c1 | c.x c.y, four Montgomery words
    each) -> the eight 32-byte big-endian canonical words a.x, a.y, b.x.c1, b.x.c0, b.y.c1, b.y.c0, c.x, c.y"""
    w = oc.fr_to_ints(np.asarray(proof_words_mont, dtype=np.uint64).reshape(8, 4), mod=opy.P)
    out = b""
    for t in range(8):
        slot = t ^ 1 if 2 <= t < 6 else t
        out += int(w[slot]).to_bytes(32, "big")
    return out


def test_the_encoding_round_trips_the_golden_proof():
    gold = json.load(open(vr.GOLDEN_JSON))
    assert gold["proof_word_order"] == ["a.x", "a.y", "b.x.c1", "b.x.c0", "b.y.c1", "b.y.c0", "c.x", "c.y"]
    words = [int(v) for v in gold["proof_words"]]
    assert all(0 <= v < opy.P for v in words)
    ax, ay, bx1, bx0, by1, by0, cx, cy = words
    struct = oc.fr_from_ints([ax, ay, bx0, bx1, by0, by1, cx, cy], mod=opy.P).reshape(32)      # the struct's order: c0 before c1
    blob = encode(struct)
    assert len(blob) == 256 and blob == vr.make_blob_words(words)
    assert [blob[32 * k:32 * k + 32].hex() for k in range(8)] == ["%064x" % v for v in words]
    assert vr.parse_blob(blob) == words
    assert encode(np.zeros(32, dtype=np.uint64)) == bytes(256)                                  # infinity: all-zero coordinates
