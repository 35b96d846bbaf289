"""The restatement of the Baby Jubjub layer (tests/ed_ref.py) against the reference's golden numbers and against itself, and the
argument checks of the new entry points -- everything here runs without a GPU."""
import ctypes
import os
import random

import numpy as np
import pytest

import ed_ref as e

Q, L, G = e.Q, e.L, e.G


@pytest.fixture(scope="module")
def g():
    return e.golden()


def test_the_fixture_matches_its_hash():
    assert e.sha256_of(e.GOLDEN_JSON) == e.GOLDEN_SHA256
    readme = open(os.path.join(e.GOLDEN, "README_cp.md")).read()
    assert e.GOLDEN_SHA256 in readme


def test_curve_constants():
    assert e.D * 168700 % Q == 168696
    assert pow(e.D, (Q - 1) // 2, Q) == Q - 1                      # d is a non-square: the unified law is complete
    assert L.bit_length() == 251 and (1 << 256) // L == 42
    assert e.on_curve(G) and e.classify(G) == e.OK and e.mul(L, G) == e.IDENTITY
    assert e.mul(8 * L, (Q - 1, 0)) == e.IDENTITY                   # the cofactor


def test_golden_aggregate_keys(g):
    assert all(e.classify(k) == e.OK for k in g["keys"])
    assert e.aggregate_keys(g["keys"]) == g["keys_sum"]


def test_golden_unmask(g):
    m = g["unmask_masked"]
    assert all(e.classify(p) == e.OK for p in g["unmask_reveals"] + [(m[0], m[1]), (m[2], m[3])])
    assert e.unmask((m[0], m[1]), g["unmask_reveals"])[1] == g["unmask_y"]


def test_golden_reveal_proof_is_accepted(g):
    st = e.golden_statement(g)
    a, b, r = e.parse_proof(g["proof"])
    assert r < L and (st[0], st[1]) == G                            # the degenerate case: e1 is the generator, so reveal = pk and a = b
    assert (st[2], st[3]) == (st[4], st[5]) and a == b
    verdict, c = e.verify(st, g["proof"], want_challenge=True)
    assert verdict == e.OK and 0 <= c < L
    assert len(e.transcript_bytes(G, G, G, a, b)) == 448


@pytest.mark.parametrize("word", range(5))
def test_golden_proof_with_a_word_changed_by_one_is_rejected(g, word):
    w = [int.from_bytes(g["proof"][32 * k:32 * k + 32], "big") for k in range(5)]
    w[word] += 1
    blob = b"".join(v.to_bytes(32, "big") for v in w)
    assert e.verify(e.golden_statement(g), blob) != e.OK


@pytest.mark.parametrize("word", range(6))
def test_golden_statement_with_a_word_changed_by_one_is_rejected(g, word):
    st = list(e.golden_statement(g))
    st[word] += 1
    assert e.verify(tuple(st), g["proof"]) != e.OK


def test_prove_then_verify_round_trips():
    rng = random.Random(7)
    for _ in range(4):
        sk, omega = rng.randrange(1, L), rng.randrange(L)
        e1 = e.mul(rng.randrange(2, L), G)
        reveal, blob = e.prove(sk, e1, omega)
        st = (*e1, *reveal, *e.keypair_public(sk))
        assert e1 != G and e.verify(st, blob) == e.OK
        a, b, r = e.parse_proof(blob)
        assert e.verify(st, e.make_proof(a, b, r + L)) == e.OK     # r is any 256-bit integer
        assert e.verify(st, e.make_proof(a, b, (r + 1) % L)) == e.EQ1_FAILS
        other = e.keypair_public(sk + 1)
        assert e.verify((*e1, *reveal, *other), blob) in (e.EQ1_FAILS, e.EQ2_FAILS)
    # verdict 5: the first equation holds, the second does not (b replaced by another subgroup point leaves c changed: build it directly)
    sk, omega, e1 = 5, 9, e.mul(3, G)
    reveal, pk, a = e.mul(sk, e1), e.mul(sk, G), e.mul(omega, e1)
    b_bad = e.mul(omega + 1, G)
    c = e.challenge(e1, reveal, pk, a, b_bad)
    assert e.verify((*e1, *reveal, *pk), e.make_proof(a, b_bad, (omega + c * sk) % L)) == e.EQ2_FAILS


def test_verdict_order():
    sk, omega, e1 = 11, 13, e.mul(17, G)
    reveal, blob = e.prove(sk, e1, omega)
    pk = e.keypair_public(sk)
    a, b, r = e.parse_proof(blob)
    off = (2, 3)
    assert not e.on_curve(off)
    low = e.add(G, e.ORDER2)
    assert e.verify((e1[0] + Q, e1[1], *reveal, *pk), blob) == e.NOT_CANONICAL
    assert e.verify((*e1, *reveal, *pk), e.make_proof((a[0], a[1] + Q), b, r)) == e.NOT_CANONICAL
    assert e.verify((*off, *reveal, *pk), e.make_proof(a, (b[0], b[1] + Q), r)) == e.NOT_CANONICAL     # 1 comes before 2
    assert e.verify((*e1, *off, *pk), blob) == e.OFF_CURVE
    assert e.verify((*low, *off, *pk), blob) == e.OFF_CURVE                                              # 2 comes before 3
    assert e.verify((*e1, *reveal, *low), blob) == e.NOT_IN_SUBGROUP
    assert e.verify((*e1, *reveal, *pk), e.make_proof(a, low, r)) == e.NOT_IN_SUBGROUP


def test_unified_law_agrees_with_the_separate_affine_formulas():
    rng = random.Random(3)
    p, q = e.mul(rng.randrange(1, L), G), e.mul(rng.randrange(1, L), G)
    assert e.add(p, q) == e.affine_add_distinct(p, q)
    assert e.add(p, p) == e.affine_double(p) == e.mul(2, p)
    assert e.add(p, e.neg(p)) == e.IDENTITY
    assert e.add(p, e.IDENTITY) == p and e.add(e.IDENTITY, p) == p and e.add(e.IDENTITY, e.IDENTITY) == e.IDENTITY
    o2 = e.ORDER2
    assert e.on_curve(o2) and e.add(o2, o2) == e.IDENTITY == e.affine_double(o2) and e.classify(o2) == e.NOT_IN_SUBGROUP
    for o4 in e.ORDER4:
        assert e.on_curve(o4) and e.add(o4, o4) == o2 == e.affine_double(o4) and e.mul(4, o4) == e.IDENTITY
        assert e.add(p, o4) == e.affine_add_distinct(p, o4)
    assert e.add(e.ORDER4[0], e.ORDER4[1]) == e.IDENTITY
    assert e.add(p, o2) == e.affine_add_distinct(p, o2) == ((-p[0]) % Q, (-p[1]) % Q)
    o8 = e.order8_point()
    assert e.on_curve(o8) and e.mul(8, o8) == e.IDENTITY and e.mul(4, o8) == o2
    assert e.add(o8, o8) == e.affine_double(o8)


def test_generator_plus_the_point_of_order_two():
    p = e.add(G, e.ORDER2)
    assert e.on_curve(p) and e.classify(p) == e.NOT_IN_SUBGROUP
    assert e.mul(2, p) == e.mul(2, G)


def test_classification():
    assert e.classify(e.IDENTITY) == e.OK
    assert e.classify((Q, 1)) == e.NOT_CANONICAL and e.classify((0, Q + 1)) == e.NOT_CANONICAL
    assert e.classify((2, 3)) == e.OFF_CURVE and e.classify((0, 0)) == e.OFF_CURVE      # the contract's infinity is no point here
    assert e.classify(e.ORDER4[0]) == e.NOT_IN_SUBGROUP and e.classify(e.order8_point()) == e.NOT_IN_SUBGROUP


def test_challenge_reduction_at_its_edges():
    for v in (0, L - 1, L, 42 * L - 1, 42 * L, (1 << 256) - 1):
        r = e.reduce_digest(v)
        assert 0 <= r < L and (v - r) % L == 0 and (v - r) // L <= 42
    assert e.reduce_digest(L - 1) == L - 1 and e.reduce_digest(L) == 0 and e.reduce_digest(42 * L - 1) == L - 1 and e.reduce_digest(42 * L) == 0
    assert e.reduce_digest((1 << 256) - 1) == (1 << 256) - 1 - 42 * L


def test_scalar_multiplication_is_by_the_integer():
    """s is not reduced: on a point outside the prime subgroup s P and (s mod L) P differ"""
    p = e.add(G, e.ORDER2)
    assert e.mul(L + 1, p) != e.mul(1, p) and e.mul(L + 1, G) == G
    assert e.mul(0, p) == e.IDENTITY and e.mul((1 << 256) - 1, G) == e.mul(((1 << 256) - 1) % L, G)


def test_wire_helpers_round_trip():
    pts = [G, e.IDENTITY, e.ORDER2]
    assert e.points_unwire(e.points_wire(pts)) == pts
    from uzkge_amd import reveal as rv
    assert np.array_equal(rv.points_to_wire(pts), e.points_wire(pts)) and rv.points_from_wire(e.points_wire(pts)) == pts
    assert (rv.Q, rv.L, rv.GENERATOR) == (Q, L, G)
    assert np.array_equal(rv.scalars_to_wire([L, 1]), e.scalars_wire([L, 1]))
    with pytest.raises(ValueError):
        rv.points_to_wire([(Q, 0)])


def test_entry_points_check_their_arguments_before_the_device():
    from uzkge_amd import UzkgeError, _native as N, backend as b
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    pts, sc, out = e.points_wire([G, G]), e.scalars_wire([1, 2]), np.zeros((2, 8), dtype=np.uint64)
    st8 = np.zeros(8, dtype=np.uint8)
    blob = np.zeros(160, dtype=np.uint8)
    bad = pts.copy()
    bad[1, 4:8] = e.raw_wire([Q])[0]                                 # y of the second point is q itself
    E = N.UZK_ERR_PARAMETER
    assert N.lib.uzk_ed_check_points(P(pts), 0, P(st8)) == E and N.lib.uzk_ed_check_points(None, 2, P(st8)) == E
    assert N.lib.uzk_ed_check_points(P(pts), N.ED_MAX_BATCH + 1, P(st8)) == E
    assert N.lib.uzk_ed_mul_batch(P(pts), 1, P(sc), 0, P(out)) == E and N.lib.uzk_ed_mul_batch(P(pts), 2, P(sc), 2, P(out)) == E
    assert N.lib.uzk_ed_mul_batch(P(pts), 1, None, 2, P(out)) == E
    assert N.lib.uzk_ed_mul_batch(P(bad), 1, P(sc), 2, P(out)) == E
    assert N.lib.uzk_ed_sum_batch(P(pts), 0, 2, P(out)) == E and N.lib.uzk_ed_sum_batch(P(pts), 1, 0, P(out)) == E
    assert N.lib.uzk_ed_sum_batch(P(bad), 2, 1, P(out)) == E and N.lib.uzk_ed_sum_batch(P(pts), 1025, 1, P(out)) == E
    assert N.lib.uzk_ed_unmask_batch(P(pts), P(bad), 1, 2, P(out)) == E and N.lib.uzk_ed_unmask_batch(P(bad), P(pts), 1, 2, P(out)) == E
    assert N.lib.uzk_ed_unmask_batch(None, P(pts), 1, 2, P(out)) == E
    assert N.lib.uzk_cp_reveal_prove_batch(P(sc), P(pts), P(sc), 0, P(out), P(out), P(blob)) == E
    assert N.lib.uzk_cp_reveal_prove_batch(P(sc), P(bad), P(sc), 2, P(out), P(out), P(blob)) == E
    assert N.lib.uzk_cp_reveal_prove_batch(None, P(pts), P(sc), 2, P(out), P(out), P(blob)) == E
    assert N.lib.uzk_cp_reveal_verify_batch(P(pts), P(blob), 0, P(st8), None) == E
    assert N.lib.uzk_cp_reveal_verify_batch(P(pts), P(blob), N.CP_MAX_BATCH + 1, P(st8), None) == E
    assert N.lib.uzk_cp_reveal_verify_batch(P(pts), None, 1, P(st8), None) == E
    with pytest.raises(UzkgeError) as err:
        b.ed_mul_batch(bad, sc)
    assert "points[1]" in str(err.value) and "y coordinate" in str(err.value)
    if b.device_count() == 0:                                        # no CPU fallback behind the new calls either
        with pytest.raises(UzkgeError) as err:
            b.ed_mul_batch(pts, sc)
        assert err.value.kind == "DeviceError"
        with pytest.raises(UzkgeError) as err:
            b.cp_reveal_verify_batch(np.zeros((1, 6, 4), dtype=np.uint64), bytes(160))
        assert err.value.kind == "DeviceError"


def test_the_kernels_scalar_side_on_the_host_under_sanitizers(g, tmp_path):
    """ed29.hpp's reduction mod L, multiply-add mod L and transcript digest are plain C++ shared by host and device: compiled here with
    g++ under AddressSanitizer and UBSan into a stand-alone program (tests/cpp/ed_scalar_host.cpp) and held to Python integers."""
    import subprocess
    from plonk_golden_verifier import keccak256
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "ed_scalar_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(root, "uzkge_amd", "csrc"),
                    os.path.join(root, "tests", "cpp", "ed_scalar_host.cpp"), "-o", exe], check=True)
    h = lambda v: "%064x" % v

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))   # nothing is allocated
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        return int(r.stdout, 16)

    for v in (0, L - 1, L, 42 * L - 1, 42 * L, (1 << 256) - 1, 17 * L + 5):
        assert run("mod", h(v)) == e.reduce_digest(v), v
    rng = random.Random("ed-scalar-host")
    for w, c, s in [(0, 0, 0), (L - 1, L - 1, L - 1), (0, L - 1, 1), (L - 1, 0, L - 1)] + [tuple(rng.randrange(L) for _ in range(3)) for _ in range(4)]:
        assert run("mad", h(w), h(c), h(s)) == (w + c * s) % L
    st = e.golden_statement(g)
    a, b, _ = e.parse_proof(g["proof"])
    words = [st[0], st[1], *G, st[2], st[3], st[4], st[5], *a, *b]
    assert run("dig", *[h(x) for x in words]) == int.from_bytes(keccak256(e.transcript_bytes(st[0:2], st[2:4], st[4:6], a, b)), "big")
    p, q = e.mul(77, G), e.mul(99, G)
    words = [*p, *G, *q, *e.ORDER2, *e.IDENTITY, *q]
    assert run("dig", *[h(x) for x in words]) == int.from_bytes(keccak256(e.transcript_bytes(p, q, e.ORDER2, e.IDENTITY, q)), "big")
