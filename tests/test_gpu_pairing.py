"""GPU: the pairing on the device (csrc/fq12_29.hpp, pairing.hip) against oracle/bn254_pairing.py, bit-exact on canonical words: every
Fq12 operation of the lane groups (uzk_test_fq12_kat), the Miller loop (uzk_test_miller: compared AFTER the oracle's final
exponentiation -- the projective lines differ from the oracle's by factors in Fq2), and uzk_pairing_product at the sizes where the
kernels change shape, at the batch limit, with points at infinity, with bad points, on a second context."""
import random

import numpy as np
import pytest

import bn254_pairing as op
import bn254_py as opy
import pairing_cases as pc
import pairing_ref as pr

pytestmark = pytest.mark.gpu
P, R = op.P, op.R
PER_WAVE = pc.header_constant("UZK_PAIRING_PAIRS_PER_WAVE", "uzkge_gpu_test.h")       # = pairs per workgroup: a workgroup is one wave
RADIX = pc.header_constant("UZK_PAIRING_TREE_RADIX", "uzkge_gpu_test.h")
MAX_PAIRS = pc.header_constant("UZK_PAIRING_MAX_PAIRS")
OPS = dict(mul=0, sqr=1, sparse=2, conj=3, frob1=4, frob2=5, frob3=6, inv=7, cyc=8, easy=9, hard=10)


@pytest.fixture(scope="module")
def elems():
    rng = random.Random("gpu-pairing-elems")
    return [pc.rand_f12(rng) for _ in range(4)] + pc.edge_f12()


def _kat(gpu, op_name, a, b=None):
    return pc.gt_from_wire(gpu.fq12_kat(OPS[op_name], pc.gt_to_wire(a), None if b is None else pc.gt_to_wire(b)))


def test_fq12_products(gpu, elems):
    b = elems[1:] + elems[:1]
    assert _kat(gpu, "mul", elems, b) == [op.f12_mul(x, y) for x, y in zip(elems, b)]
    assert _kat(gpu, "sqr", elems) == [op.f12_mul(x, x) for x in elems]
    lines = [[y[0], y[1], (0, 0), y[3], (0, 0), (0, 0)] for y in b]
    assert _kat(gpu, "sparse", elems, b) == [op.f12_mul(x, l) for x, l in zip(elems, lines)]      # b's other coefficients are ignored


def test_fq12_conjugation_and_frobenius(gpu, elems):
    assert _kat(gpu, "conj", elems) == [pr.f12_conj(x) for x in elems]
    for j in (1, 2, 3):
        got = _kat(gpu, "frob%d" % j, elems)
        assert got == [pr.f12_frob(x, j) for x in elems]
        assert got[0] == op.f12_pow(elems[0], P ** j)                  # the oracle itself, once per map
    assert _kat(gpu, "conj", elems[:1])[0] == op.f12_pow(elems[0], P ** 6)


def test_fq12_inverse(gpu, elems):
    """inverse . element = 1; the inverse of 0 is 0 (documented in fq12_29.hpp and the test header)"""
    inv = _kat(gpu, "inv", elems)
    assert inv == [pr.f12_inv(x) for x in elems]
    for x, y in zip(elems, _kat(gpu, "mul", inv, elems)):
        assert y == (pc.ONE if any(c != (0, 0) for c in x) else [(0, 0)] * 6)
    assert inv[4] == [(0, 0)] * 6 and elems[4] == [(0, 0)] * 6


def test_cyclotomic_square_and_the_final_exponentiation_parts(gpu, elems):
    """the Granger-Scott square on outputs of the easy part only, against the plain square; the hard part against the exact power"""
    src = elems[:4] + elems[6:8]
    easy = _kat(gpu, "easy", src)
    assert easy == [pr.easy_part(x) for x in src]
    assert _kat(gpu, "cyc", easy) == _kat(gpu, "sqr", easy) == [op.f12_mul(x, x) for x in easy]
    hard = _kat(gpu, "hard", easy[:2])
    assert hard[0] == op.f12_pow(easy[0], pr.HARD) == op.final_exponentiation(src[0])
    assert hard[1] == pr.hard_part(easy[1])


def test_miller_values_after_the_oracles_final_exponentiation(gpu):
    g, h = opy.G1_GEN, op.G2_GEN
    y = pow(2, (P + 1) // 4, P)
    assert y * y % P == 2                                              # (p - 1, sqrt 2) is on y^2 = x^3 + 3
    pts = [(g, h), (opy.g1_mul(g, 5), op.g2_mul(h, 7)), ((P - 1, y), op.g2_mul(h, R - 1)), (opy.g1_mul(g, R - 2), op.g2_mul(h, 3))]
    got = pc.gt_from_wire(gpu.miller_loops(pc.p_wire([p for p, _ in pts]), pc.q_wire([q for _, q in pts])))
    e = pc.e_gh()
    want = [e, op.f12_pow(e, 35), op.pairing(*pts[2]), op.f12_pow(e, (R - 2) * 3 % R)]
    for f, w in zip(got, want):
        assert op.final_exponentiation(f) == w
    inf = gpu.miller_loops(pc.p_wire([None, g]), pc.q_wire([h, None]))
    assert pc.gt_from_wire(inf) == [pc.ONE, pc.ONE]


def _product(gpu, p, q):
    gt, one = gpu.pairing_product(p, q)
    return pc.gt_from_wire(gt)[0], one


def test_products_of_up_to_three_pairs_against_the_oracle(gpu):
    g, h, e = opy.G1_GEN, op.G2_GEN, pc.e_gh()
    assert _product(gpu, pc.p_wire([]), pc.q_wire([])) == (pc.ONE, True)
    assert _product(gpu, pc.p_wire([g]), pc.q_wire([h])) == (e, False)
    a, b = 0x1234567, 0x89abcdef0123
    lhs = _product(gpu, pc.p_wire([opy.g1_mul(g, a)]), pc.q_wire([op.g2_mul(h, b)]))
    assert lhs == _product(gpu, pc.p_wire([opy.g1_mul(g, a * b)]), pc.q_wire([h])) == (op.f12_pow(e, a * b), False)     # e(aG, bH) = e(abG, H)
    p5 = opy.g1_mul(g, 5)
    assert _product(gpu, pc.p_wire([p5, opy.g1_neg(p5)]), pc.q_wire([op.g2_mul(h, 9)] * 2)) == (pc.ONE, True)          # e(P, Q) e(-P, Q) = 1
    pairs = [(opy.g1_mul(g, 3), op.g2_mul(h, 11)), (opy.g1_mul(g, R - 7), h), (g, op.g2_mul(h, 2))]
    f = pc.ONE
    for p, q in pairs:
        f = op.f12_mul(f, op.miller_loop(p, q))
    want = op.final_exponentiation(f)
    assert want == op.f12_pow(e, (33 - 7 + 2) % R)
    assert _product(gpu, pc.p_wire([p for p, _ in pairs]), pc.q_wire([q for _, q in pairs])) == (want, False)


@pytest.mark.parametrize("n", sorted({PER_WAVE - 1, PER_WAVE, PER_WAVE + 1, RADIX * RADIX - 1, RADIX * RADIX, RADIX * RADIX + 1}))
def test_sizes_around_a_wave_of_pairs_and_a_level_of_the_tree(gpu, n):
    """one below, at and one above the pairs of a wave (PER_WAVE = the pairs of a workgroup: a workgroup is one wave) and a full
    second level of the tree of radix RADIX"""
    p, q, s = pc.log_pairs(n, "edge")
    assert _product(gpu, p, q) == (pc.expected_power(s), False)


@pytest.mark.parametrize("n", [55, MAX_PAIRS])
def test_a_deck_and_the_batch_limit_by_the_closed_form(gpu, n):
    p, q, s = pc.log_pairs(n, "zero", total=0)
    assert s == 0 and _product(gpu, p, q) == (pc.ONE, True)
    p[0] = pc.p_wire([opy.G1_GEN])[0]                                  # a_0 := 1: the sum moves by 1 - a_0
    s = (1 - pc.logs_of(n, "zero", total=0)[0]) % R
    assert s != 0 and _product(gpu, p, q) == (pc.expected_power(s), False)


def test_refusals(gpu):
    from uzkge_amd import UzkgeError
    p, q, _ = pc.log_pairs(5, "refusals")
    with pytest.raises(UzkgeError) as e:
        gpu.pairing_product(np.zeros((MAX_PAIRS + 1, 8), dtype=np.uint64), np.zeros((MAX_PAIRS + 1, 16), dtype=np.uint64))
    assert e.value.kind == "ParameterError"
    bad_coord = p.copy()
    bad_coord[3, :4] = np.array([(P >> (64 * k)) & (2 ** 64 - 1) for k in range(4)], dtype=np.uint64)       # the words of p itself
    off_p = p.copy()
    off_p[2, 4:] = p[1, 4:]                                            # another point's y
    off_q = q.copy()
    off_q[4, 8:] = q[0, 8:]
    bad_q_coord = q.copy()
    bad_q_coord[1, 4:8] = bad_coord[3, :4]
    for pp, qq, index, text in ((bad_coord, q, 3, "not below p"), (off_p, q, 2, "not on its curve"), (p, off_q, 4, "not on its curve"),
                                (p, bad_q_coord, 1, "not below p")):
        with pytest.raises(UzkgeError) as e:
            gpu.pairing_product(pp, qq)
        assert e.value.kind == "ParameterError" and ("pair %d:" % index) in str(e.value) and text in str(e.value), str(e.value)
    both = bad_coord.copy()
    both[2, 4:] = p[1, 4:]
    with pytest.raises(UzkgeError) as e:
        gpu.pairing_product(both, q)
    assert "pair 2:" in str(e.value)                                   # the FIRST bad index
    assert _product(gpu, p, q)[1] is False                             # and the context still works


def test_points_at_infinity_contribute_one(gpu):
    n = 9
    p, q, total = pc.log_pairs(n, "inf")
    logs = pc.logs_of(n, "inf")                                        # the a_i themselves, to leave one out of the sum
    assert sum(x * (i + 1) for i, x in enumerate(logs)) % R == total
    for pos in (0, n // 2, n - 1):
        for what in ("p", "q", "both"):
            pp, qq = p.copy(), q.copy()
            if what in ("p", "both"):
                pp[pos] = 0
            if what in ("q", "both"):
                qq[pos] = 0
            s = sum(x * (i + 1) for i, x in enumerate(logs) if i != pos) % R
            assert _product(gpu, pp, qq) == (pc.expected_power(s), False), (pos, what)
    assert _product(gpu, np.zeros((3, 8), dtype=np.uint64), q[:3]) == (pc.ONE, True)


def test_gt_out_is_optional(gpu):
    p, q, _ = pc.log_pairs(3, "null", total=0)
    gt, one = gpu.pairing_product(p, q, want_gt=False)
    assert gt is None and one is True
    gt, one = gpu.pairing_product(p[:2], q[:2], want_gt=False)
    assert gt is None and one is False


def test_second_context_and_repeated_calls_give_identical_bytes(gpu):
    p, q, s = pc.log_pairs(11, "ctx")
    first, _ = gpu.pairing_product(p, q)
    again, _ = gpu.pairing_product(p, q)
    assert np.array_equal(first, again) and pc.gt_from_wire(first)[0] == pc.expected_power(s)
    h = gpu.ctx_create()
    try:
        gpu.ctx_set_current(h)
        other, _ = gpu.pairing_product(p, q)
        small, _ = gpu.pairing_product(p[:2], q[:2])
        other2, _ = gpu.pairing_product(p, q)                          # the workspace does not shrink or move results
    finally:
        gpu.ctx_set_current(0)
        gpu.ctx_destroy(h)
    assert np.array_equal(first, other) and np.array_equal(first, other2) and not np.array_equal(first, small)
    assert np.array_equal(first, gpu.pairing_product(p, q)[0])
