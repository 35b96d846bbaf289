"""GPU: PlonkVerifierKey.verify_batch -- uzk_verify_fold, two conversions to affine and uzk_pairing_product over (L, [tau] H), (-R, H)
-- accepts the golden 52-card proof and rejects a tampered one, against tests/plonk_batch_ref.py."""
import pytest

import plonk_batch_ref as br
import plonk_golden_verifier as gv

pytestmark = pytest.mark.gpu


def test_golden_52_card_proof_is_accepted_and_a_tampered_one_rejected(gpu):
    from uzkge_amd.poly_commit import PlonkVerifierKey
    g2 = br.load_g2()
    vk, proof, pi = gv.load_golden(52)
    key = PlonkVerifierKey(vk, br.prefix(52))
    try:
        raw = gv.proof_to_bytes(proof)
        accepted, status = key.verify_batch([raw], [pi], None, g2[0], g2[1])
        assert accepted is True and list(status) == [0]
        left, right = br.fold([br.terms(vk, proof, pi, br.prefix(52))], [1])
        assert br.accepts(left, right, g2)
        bad_pi = list(pi)
        bad_pi[0] = (bad_pi[0] + 1) % br.R
        accepted, status = key.verify_batch([raw, raw], [pi, bad_pi], [3, 5], g2[0], g2[1])
        assert accepted is False and list(status) == [0, 0]
        l2, r2 = br.fold([br.terms(vk, proof, pi, br.prefix(52)), br.terms(vk, proof, bad_pi, br.prefix(52))], [3, 5])
        assert not br.accepts(l2, r2, g2)
        accepted, status = key.verify_batch([raw, raw], [pi, pi], [3, 5], g2[0], g2[1])
        assert accepted is True and list(status) == [0, 0]
        accepted, _ = key.verify_batch([raw], [pi], None, g2[1], g2[0])          # the two G2 elements swapped
        assert accepted is False
    finally:
        key.release()
