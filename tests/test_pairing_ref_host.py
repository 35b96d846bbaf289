"""CPU: tests/pairing_ref.py -- the Python-integer restatement of the DEVICE's pairing (one output coefficient per lane, the sparse line
product, the Granger-Scott square, the norm-chain inverse, projective Miller steps, the exact hard part) -- held to
oracle/bn254_pairing.py; the argument checks of uzk_pairing_product and uzk_g16_verify_batch that answer before a device is touched;
the header's constants."""
import ctypes
import random

import numpy as np

import bn254_pairing as op
import bn254_py as opy
import pairing_cases as pc
import pairing_ref as pr

P, R = op.P, op.R


def _elems():
    rng = random.Random("pairing-ref-host")
    return [pc.rand_f12(rng) for _ in range(3)] + pc.edge_f12()


def test_products_match_the_oracle_on_random_and_edge_elements():
    es = _elems()
    for i, a in enumerate(es):
        b = es[(i + 1) % len(es)]
        assert pr.f12_mul(a, b) == op.f12_mul(a, b)
        assert pr.f12_sqr(a) == op.f12_mul(a, a)
        ell = [b[0], b[1], (0, 0), b[3], (0, 0), (0, 0)]
        assert pr.f12_mul_sparse(a, (b[0], b[1], b[3])) == op.f12_mul(a, ell)
    assert pr.f12_mul(es[0], pr.F12_ONE) == es[0]


def test_conjugation_and_frobenius_match_powers():
    es = _elems()[:5]
    for a in es:
        assert pr.f12_conj(a) == op.f12_pow(a, P ** 6)
    for a in es[:2]:
        for j in (1, 2, 3):
            assert pr.f12_frob(a, j) == op.f12_pow(a, P ** j)


def test_frobenius_constants_are_powers_of_w():
    w = [(0, 0), (1, 0)] + [(0, 0)] * 4
    for j in (1, 2, 3):
        wp = op.f12_pow(w, P ** j)                    # = gamma_j,1 w
        assert wp == [(0, 0), pr.GAMMA[j][1]] + [(0, 0)] * 4
        for k in range(6):
            assert pr.GAMMA[j][k] == op.f2_pow(pr.GAMMA[j][1], k) == op.f2_pow(op.XI, k * (P ** j - 1) // 6)
    assert (pr.GAMMA[1][2], pr.GAMMA[1][3], pr.GAMMA[2][2], pr.GAMMA[2][3]) == (op.G12, op.G13, op.G22, op.G23)


def test_inverse_by_the_norm_chain():
    for a in _elems():
        inv = pr.f12_inv(a)
        if all(c == (0, 0) for c in a):
            assert inv == a                            # the inverse of 0 is 0
        elif op.f12_mul(a, op.f12_pow(a, P ** 12 - 2)) == pr.F12_ONE:
            assert op.f12_mul(inv, a) == pr.F12_ONE
        else:                                          # a zero divisor cannot occur in a field
            raise AssertionError(a)


def test_cyclotomic_square_on_outputs_of_the_easy_part():
    rng = random.Random("pairing-ref-cyc")
    for _ in range(3):
        e = pr.easy_part(pc.rand_f12(rng))
        assert pr.f12_cyc_sqr(e) == op.f12_mul(e, e)
        assert op.f12_mul(pr.f12_conj(e), e) == pr.F12_ONE          # inversion is conjugation there
    a = pc.rand_f12(rng)
    assert pr.f12_cyc_sqr(a) != op.f12_mul(a, a)                    # and only there


def test_hard_part_is_the_exact_exponent():
    assert pr.HARD == P ** 3 + pr.L2 * P ** 2 + pr.L1 * P + pr.L0
    e = pr.easy_part(pc.rand_f12(random.Random("pairing-ref-hard")))
    assert pr.hard_part(e) == op.f12_pow(e, pr.HARD)


def test_final_exponentiation_equals_the_oracles():
    rng = random.Random("pairing-ref-fe")
    for _ in range(3):
        a = pc.rand_f12(rng)
        assert pr.final_exponentiation(a) == op.final_exponentiation(a)


def test_miller_values_agree_after_the_final_exponentiation():
    g = opy.G1_GEN
    pairs = [(g, op.G2_GEN), (opy.g1_mul(g, 5), op.g2_mul(op.G2_GEN, 7)), (opy.g1_mul(g, R - 1), op.g2_mul(op.G2_GEN, 12345678901234567890))]
    for p, q in pairs:
        assert op.final_exponentiation(pr.miller_loop(p, q)) == op.pairing(p, q)
    assert pr.miller_loop(None, op.G2_GEN) == pr.F12_ONE and pr.miller_loop(g, None) == pr.F12_ONE
    assert pr.pairing_product([(g, op.G2_GEN), (opy.g1_neg(g), op.G2_GEN)]) == pr.F12_ONE


def test_header_constants():
    assert pc.header_constant("UZK_PAIRING_MAX_PAIRS") == pc.header_constant("UZK_G16_VERIFY_MAX_BATCH") + 3 == 4099
    from uzkge_amd import _native as N
    assert N.PAIRING_MAX_PAIRS == 4099
    assert pc.header_constant("UZK_PAIRING_PAIRS_PER_WAVE", "uzkge_gpu_test.h") >= 1


def test_entry_points_check_their_arguments_before_the_device():
    from uzkge_amd import _native as N
    lib = N.lib
    buf = np.zeros(4200 * 16, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    one = ctypes.c_int(7)
    assert lib.uzk_pairing_product(p, p, N.PAIRING_MAX_PAIRS + 1, p, ctypes.byref(one)) == N.UZK_ERR_PARAMETER
    assert b"4100" in lib.uzk_last_error()
    assert lib.uzk_pairing_product(None, p, 1, p, ctypes.byref(one)) == N.UZK_ERR_PARAMETER
    assert lib.uzk_pairing_product(p, None, 1, p, ctypes.byref(one)) == N.UZK_ERR_PARAMETER
    assert lib.uzk_pairing_product(p, p, 1, p, None) == N.UZK_ERR_PARAMETER
    assert one.value == 7
    gt = np.ones((6, 2, 4), dtype=np.uint64)
    assert lib.uzk_pairing_product(None, None, 0, gt.ctypes.data_as(ctypes.c_void_p), ctypes.byref(one)) == N.UZK_OK    # the empty product: no device
    assert one.value == 1 and pc.gt_from_wire(gt) == [pc.ONE]
    assert lib.uzk_pairing_product(None, None, 0, None, ctypes.byref(one)) == N.UZK_OK
    ok = ctypes.c_int(7)
    vb = lib.uzk_g16_verify_batch
    assert vb(12345, p, p, N.G16_VERIFY_MAX_BATCH + 1, p, p, p, ctypes.byref(ok)) == N.UZK_ERR_PARAMETER
    assert vb(12345, p, p, 2, None, p, p, ctypes.byref(ok)) == N.UZK_ERR_PARAMETER          # a batch without weights
    assert vb(12345, p, p, 1, p, None, p, ctypes.byref(ok)) == N.UZK_ERR_PARAMETER
    assert vb(12345, p, p, 1, p, p, None, ctypes.byref(ok)) == N.UZK_ERR_PARAMETER
    assert vb(12345, p, p, 1, p, p, p, None) == N.UZK_ERR_PARAMETER
    assert vb(12345, p, p, 1, p, p, p, ctypes.byref(ok)) == N.UZK_ERR_PARAMETER             # an unknown key
    assert b"unknown verifying key" in lib.uzk_last_error() and ok.value == 7
    assert lib.uzk_test_fq12_kat(99, p, p, p, 1) == N.UZK_ERR_PARAMETER
    assert lib.uzk_test_miller(p, p, N.PAIRING_MAX_PAIRS + 1, p) == N.UZK_ERR_PARAMETER
