"""The restatement of the mask and the remask (tests/shuffle_ref.py) against the reference's preprocessed tables and against itself,
and the argument checks of the six new entry points -- everything here runs without a GPU."""
import ctypes
import os
import random

import numpy as np
import pytest

import ed_ref as e
import shuffle_ref as s

Q, L, G = e.Q, e.L, e.G


@pytest.fixture(scope="module")
def pk():
    return e.mul(0x1234567, G)


@pytest.fixture(scope="module")
def t_pk(pk):
    return s.tables(pk)


def test_the_fixture_matches_its_hash():
    assert e.sha256_of(s.TABLES_JSON) == s.TABLES_SHA256
    assert s.TABLES_SHA256 in open(os.path.join(e.GOLDEN, "README_shuffle.md")).read()


def test_tables_reproduce_the_references_twelve_numbers():
    """x, y and dxy of the entries (0,0), (0,3), (1,0), (83,3): the reference's dxy IS d x y of the affine point"""
    gold, t = s.golden_tables(), s.generator_tables()
    assert sorted(gold) == [(0, 0), (0, 3), (1, 0), (83, 3)]
    for (i, j), want in gold.items():
        assert s.entry(t[i][j]) == want, (i, j)
    assert t[0][0] == G


def test_tables_are_the_multiples_they_are_defined_as(pk, t_pk):
    for t, p in ((s.generator_tables(), G), (t_pk, pk)):
        for i in (0, 1, 63, 83):
            for j in range(4):
                assert t[i][j] == e.mul(((j + 1) << (4 * i)) % L, p)
    assert (4 << (4 * 83)).bit_length() == 335
    # off the subgroup the definition is by the integer: a point of order 8 collapses after the first doublings
    o8 = e.order8_point()
    t8 = s.tables(o8)
    assert [t8[0][j] for j in range(4)] == [e.mul(j + 1, o8) for j in range(4)] and t8[0][3] == e.ORDER2
    assert all(t8[i][j] == e.IDENTITY for i in range(1, 84) for j in range(4))
    assert all(pt == e.IDENTITY for row in s.tables(e.IDENTITY) for pt in row)
    assert s.entry(e.IDENTITY) == (0, 1, 0)


def test_digits():
    assert [s.signed_digit(d) for d in range(8)] == [-1, -2, -3, -4, 1, 2, 3, 4]
    assert s.digit_of_bits((True, False, True)) == 5 and s.signed_digit(5) == 2          # (true, false, true): + generator[1]
    assert s.digit_of_bits((False, True, False)) == 2 and s.signed_digit(2) == -3        # (false, true, false): - generator[2]
    with pytest.raises(ValueError):
        s.signed_digit(8)
    assert s.remark_scalar([7] * 84) == 4 * ((1 << 336) - 1) // 15 and s.remark_scalar([7] * 84).bit_length() == 335      # above any 256-bit scalar
    assert s.remark_scalar([0] * 84) == -((1 << 336) - 1) // 15


@pytest.mark.parametrize("kind", ["random", "zeros", "sevens"])
def test_eval_remark_is_the_equivalent_scalar(pk, t_pk, kind):
    rng = random.Random("remark-" + kind)
    digits = {"random": [rng.randrange(8) for _ in range(84)], "zeros": [0] * 84, "sevens": [7] * 84}[kind]
    card = (e.mul(rng.randrange(1, L), G), e.mul(rng.randrange(1, L), G))
    trace = s.eval_remark_with_trace(card, digits, t_pk)
    out = s.eval_remark(card, digits, t_pk)
    assert len(trace) == 84 and trace[-1] == (out[1][0], out[1][1], out[0][0], out[0][1])
    assert out == s.remark_by_scalar(card, digits, pk)
    rho = s.remark_scalar(digits) % L
    assert out == (e.add(card[0], e.mul(rho, G)), e.add(card[1], e.mul(rho, pk)))


def test_trace_edges(pk, t_pk):
    """the first addition a doubling; trace entry 0 the identity"""
    tg = s.generator_tables()
    for j in range(4):
        rest = [5] * 83
        tr = s.eval_remark_with_trace((tg[0][j], tg[0][j]), [s.digit_for(j, True)] + rest, t_pk)
        assert (tr[0][2], tr[0][3]) == e.mul(2 * (j + 1), G)
        tr = s.eval_remark_with_trace((tg[0][j], t_pk[0][j]), [s.digit_for(j, False)] + rest, t_pk)
        assert tr[0] == (0, 1, 0, 1)


def test_shuffle_permutes_by_rows(pk, t_pk):
    rng = random.Random("shuffle-host")
    cards = [(e.mul(rng.randrange(1, L), G), e.mul(rng.randrange(1, L), G)) for _ in range(3)]
    digits = [[rng.randrange(8) for _ in range(84)] for _ in cards]
    deck, traces = s.shuffle(cards, digits, [2, 0, 1], t_pk)
    plain = [s.eval_remark(c, d, t_pk) for c, d in zip(cards, digits)]
    assert deck == [plain[2], plain[0], plain[1]] and len(traces) == 3
    assert s.shuffle(cards, digits, None, t_pk)[0] == plain


def test_mask_transcript_and_round_trip(pk):
    rng = random.Random("mask-host")
    card, r, omega = e.mul(rng.randrange(1, L), G), rng.randrange(1, L), rng.randrange(L)
    masked, blob = s.mask(pk, card, r, omega)
    a, b, _ = e.parse_proof(blob)
    t = s.mask_transcript_bytes(pk, masked[0], e.sub(masked[1], card), a, b)
    assert len(t) == 448 and t[:32] == bytes(25) + b"Masking" and t[32:64] == bytes(30) + b"DL"
    assert t[64:128] == e._w(G[0]) + e._w(G[1]) and t[128:192] == e._w(pk[0]) + e._w(pk[1])
    assert masked == (e.mul(r, G), e.add(card, e.mul(r, pk)))
    verdict, c = s.verify_mask(pk, card, masked, blob, want_challenge=True)
    assert verdict == e.OK and 0 <= c < L
    # r = 1 is the shape of init_masked_cards
    m1, blob1 = s.mask(pk, card, 1, omega)
    assert m1 == (G, e.add(card, pk)) and s.verify_mask(pk, card, m1, blob1) == e.OK
    # the same numbers under the label of a reveal are another proof
    a2, b2 = e.mul(omega, G), e.mul(omega, pk)
    c_rev = e.reduce_digest(int.from_bytes(e.keccak256(t.replace(bytes(25) + b"Masking", e._pad32(b"Revealing"), 1)), "big"))
    assert c_rev != c
    assert s.verify_mask(pk, card, masked, e.make_proof(a2, b2, (omega + c_rev * r) % L)) == e.EQ1_FAILS


def test_every_failure_verdict_of_a_mask_is_reachable(pk):
    card, r, omega = e.mul(21, G), 33, 55
    masked, blob = s.mask(pk, card, r, omega)
    a, b, rr = e.parse_proof(blob)
    off, low = (2, 3), e.add(G, e.ORDER2)
    assert s.verify_mask(pk, (card[0] + Q, card[1]), masked, blob) == e.NOT_CANONICAL
    assert s.verify_mask(pk, card, masked, e.make_proof(a, (b[0], b[1] + Q), rr)) == e.NOT_CANONICAL
    assert s.verify_mask(off, card, (masked[0], (masked[1][0], masked[1][1] + Q)), blob) == e.NOT_CANONICAL        # 1 comes before 2
    assert s.verify_mask(pk, off, masked, blob) == e.OFF_CURVE
    assert s.verify_mask(low, card, (off, masked[1]), blob) == e.OFF_CURVE                                           # 2 comes before 3
    assert s.verify_mask(low, card, masked, blob) == e.NOT_IN_SUBGROUP
    assert s.verify_mask(pk, card, masked, e.make_proof(low, b, rr)) == e.NOT_IN_SUBGROUP
    assert s.verify_mask(pk, card, masked, e.make_proof(a, b, (rr + 1) % L)) == e.EQ1_FAILS
    # the first equation holds, the second does not: b from another omega, the response over the challenge of what is sent
    b_bad = e.mul(omega + 1, pk)
    c = s.mask_challenge(pk, masked[0], e.sub(masked[1], card), a, b_bad)
    assert s.verify_mask(pk, card, masked, e.make_proof(a, b_bad, (omega + c * r) % L)) == e.EQ2_FAILS
    # another card under the same e2: the statement's second point changes
    assert s.verify_mask(pk, e.mul(22, G), masked, blob) in (e.EQ1_FAILS, e.EQ2_FAILS)


def test_entry_points_check_their_arguments_before_the_device():
    from uzkge_amd import UzkgeError, _native as N, backend as b, reveal as rv
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    E = N.UZK_ERR_PARAMETER
    pts, sc, out = e.points_wire([G, G]), e.scalars_wire([1, 2]), np.zeros((2, 8), dtype=np.uint64)
    bad = pts.copy()
    bad[1, 4:8] = e.raw_wire([Q])[0]                                 # y of the second point is q itself
    badx = pts.copy()
    badx[0, 0:4] = e.raw_wire([Q])[0]
    digits, perm = np.zeros((2, 84), dtype=np.uint8), np.array([1, 0], dtype=np.uint32)
    blob, st8, key = np.zeros(320, dtype=np.uint8), np.zeros(8, dtype=np.uint8), ctypes.c_uint64(0)
    lib = N.lib
    assert N.REMARK_ITERATIONS == s.ITERATIONS == 84
    # key_create
    assert lib.uzk_remark_key_create(None, ctypes.byref(key)) == E and lib.uzk_remark_key_create(P(pts), None) == E
    assert lib.uzk_remark_key_create(P(badx), ctypes.byref(key)) == E and lib.uzk_remark_key_create(P(bad[1:]), ctypes.byref(key)) == E
    # key_release / key_tables: unknown keys
    assert lib.uzk_remark_key_release(0) == E and lib.uzk_remark_key_release(12345) == E
    assert lib.uzk_remark_key_tables(12345, P(out), None) == E
    # remark_batch: the batch, the pointers and the key come before everything else
    assert lib.uzk_remark_batch(12345, P(pts), P(pts), P(digits), None, 0, P(out), P(out), None) == E
    assert lib.uzk_remark_batch(12345, P(pts), P(pts), P(digits), None, N.ED_MAX_BATCH + 1, P(out), P(out), None) == E
    assert lib.uzk_remark_batch(12345, None, P(pts), P(digits), None, 2, P(out), P(out), None) == E
    assert lib.uzk_remark_batch(12345, P(pts), P(bad), P(digits), P(perm), 2, P(out), P(out), None) == E
    assert b"e2[1]" in lib.uzk_last_error()
    assert lib.uzk_remark_batch(12345, P(badx), P(pts), P(digits), P(perm), 2, P(out), P(out), None) == E
    assert b"e1[0]" in lib.uzk_last_error()
    eight = digits.copy()
    eight[1, 83] = 8
    assert lib.uzk_remark_batch(12345, P(pts), P(pts), P(eight), P(perm), 2, P(out), P(out), None) == E
    assert b"digit 83 of card 1" in lib.uzk_last_error()
    for wrong in ([0, 0], [1, 1], [0, 2]):
        assert lib.uzk_remark_batch(12345, P(pts), P(pts), P(digits), P(np.array(wrong, dtype=np.uint32)), 2, P(out), P(out), None) == E
        assert b"not a permutation" in lib.uzk_last_error()
    assert lib.uzk_remark_batch(12345, P(pts), P(pts), P(digits), P(perm), 2, P(out), P(out), None) == E
    assert b"unknown remask key" in lib.uzk_last_error()
    # mask_prove
    assert lib.uzk_cp_mask_prove_batch(P(pts), P(pts), P(sc), P(sc), 0, P(out), P(out), P(blob)) == E
    assert lib.uzk_cp_mask_prove_batch(P(pts), P(pts), P(sc), P(sc), N.CP_MAX_BATCH + 1, P(out), P(out), P(blob)) == E
    assert lib.uzk_cp_mask_prove_batch(None, P(pts), P(sc), P(sc), 2, P(out), P(out), P(blob)) == E
    assert lib.uzk_cp_mask_prove_batch(P(pts), P(pts), None, P(sc), 2, P(out), P(out), P(blob)) == E
    assert lib.uzk_cp_mask_prove_batch(P(badx), P(pts), P(sc), P(sc), 2, P(out), P(out), P(blob)) == E
    assert lib.uzk_cp_mask_prove_batch(P(pts), P(bad), P(sc), P(sc), 2, P(out), P(out), P(blob)) == E
    assert b"cards[1]" in lib.uzk_last_error() and b"y coordinate" in lib.uzk_last_error()
    # mask_verify: a checking call -- coordinates are its verdicts' business, the batch and the pointers are not
    assert lib.uzk_cp_mask_verify_batch(P(pts), P(pts), P(pts), P(pts), P(blob), 0, P(st8), None) == E
    assert lib.uzk_cp_mask_verify_batch(P(pts), P(pts), P(pts), P(pts), P(blob), N.CP_MAX_BATCH + 1, P(st8), None) == E
    assert lib.uzk_cp_mask_verify_batch(P(pts), None, P(pts), P(pts), P(blob), 2, P(st8), None) == E
    assert lib.uzk_cp_mask_verify_batch(P(pts), P(pts), P(pts), P(pts), None, 2, P(st8), None) == E
    # the Python layer
    assert rv.remark_scalar([7] * 84) == s.remark_scalar([7] * 84) and rv.remark_scalar([0, 5] + [4] * 82) == s.remark_scalar([0, 5] + [4] * 82)
    with pytest.raises(ValueError):
        rv.remark_scalar([8] + [0] * 83)
    with pytest.raises(ValueError):
        rv.remark_scalar([0] * 83)
    if b.device_count() == 0:                                        # no CPU fallback behind the new calls either
        with pytest.raises(UzkgeError) as err:
            b.RemarkKey(pts[0])
        assert err.value.kind == "DeviceError"
        with pytest.raises(UzkgeError) as err:
            b.cp_mask_prove_batch(pts[0], pts, sc, sc)
        assert err.value.kind == "DeviceError"
        with pytest.raises(UzkgeError) as err:
            b.cp_mask_verify_batch(pts[0], pts, pts, pts, bytes(320))
        assert err.value.kind == "DeviceError"


def test_the_label_of_the_transcript_on_the_host_under_sanitizers(pk, tmp_path):
    """ed29.hpp's transcript digest takes its label as an argument now; it is plain C++ shared by host and device: compiled here with
    g++ under AddressSanitizer and UBSan into a stand-alone program (tests/cpp/cp_label_host.cpp) and held to Python integers."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cp_label_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(root, "uzkge_amd", "csrc"),
                    os.path.join(root, "tests", "cpp", "cp_label_host.cpp"), "-o", exe], check=True)

    def run(label, words):
        r = subprocess.run([exe, label, *["%064x" % v for v in words]], capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))                                  # nothing is allocated
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        return int(r.stdout, 16)

    card, r, omega = e.mul(77, G), 99, 1234
    (e1, e2), blob = s.mask(pk, card, r, omega)
    a, b, _ = e.parse_proof(blob)
    diff = e.sub(e2, card)
    words = [*G, *pk, *e1, *diff, *a, *b]
    t = s.mask_transcript_bytes(pk, e1, diff, a, b)
    assert run("masking", words) == int.from_bytes(e.keccak256(t), "big")
    assert run("revealing", words) == int.from_bytes(e.keccak256(e._pad32(b"Revealing") + t[32:]), "big")
    # the reveal's own order under the explicit label is what ed_ref's transcript hashes
    words = [*e1, *G, *diff, *pk, *a, *b]
    assert run("revealing", words) == int.from_bytes(e.keccak256(e.transcript_bytes(e1, diff, pk, a, b)), "big")
    edge = [Q - 1, 0] * 6
    assert run("masking", edge) == int.from_bytes(e.keccak256(e._pad32(b"Masking") + e._pad32(b"DL") + b"".join(e._w(v) for v in edge)), "big")
