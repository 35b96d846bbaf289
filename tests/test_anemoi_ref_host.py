"""The Anemoi-Jive restatement (tests/anemoi_ref.py) held to the reference's recorded answers and to itself, the generated device
constants held to the restatement, and every argument check of the uzk_anemoi_* / uzk_cp_reveal_*0 entry points -- no GPU."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import anemoi_ref as a
import ed_ref as e

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = a.R


def test_the_fixture_matches_its_hash():
    readme = open(os.path.join(ROOT, "tests", "golden", "README_anemoi.md")).read()
    want = re.search(r"([0-9a-f]{64})  anemoi_golden\.json", readme).group(1)
    assert e.sha256_of(os.path.join(ROOT, "tests", "golden", "anemoi_golden.json")) == want


def test_the_recorded_hash_and_stream_cipher_outputs():
    g = a.golden()
    assert g["input"] == [1, 2, 3, 4] and g["lengths"] == [2, 4, 6, 7] and len(g["stream"]) == 7
    assert a.eval_variable_length_hash(g["input"]) == g["hash"] == g["stream"][0]
    for n in g["lengths"]:
        assert a.eval_stream_cipher(g["input"], n) == g["stream"][:n]


def test_constants_follow_the_rule():
    assert a.G * a.DELTA % R == 1 and a.ALPHA * a.ALPHA_INV % (R - 1) == 1
    assert a.ALPHA_INV.bit_length() == 254 and bin(a.ALPHA_INV).count("1") == 136
    assert a.KEYS_X[0] == [a.G + 2 ** 5, (a.G + (1 + a.PI1) ** 5) % R]      # pi0^0 = pi1^0 = 1
    assert a.KEYS_Y[0][0] == (a.G + 2 ** 5 + a.DELTA) % R
    assert len({k for row in a.KEYS_X + a.KEYS_Y for k in row}) == 56


def test_the_generated_device_constants_are_the_restatements():
    """uzkge_amd/csrc/anemoi_consts.inc: keys, delta and g in 2^261-form limbs, the exponent's words and its 3-bit windows"""
    import subprocess
    import sys
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_anemoi_consts.py"), "--check"]).returncode == 0
    text = open(os.path.join(ROOT, "uzkge_amd", "csrc", "anemoi_consts.inc")).read()
    val = lambda body: sum(int(w, 16) << (29 * i) for i, w in enumerate(re.findall(r"0x([0-9a-f]{8})u", body)))
    keys = [val(row) for row in re.findall(r"\{((?:0x[0-9a-f]{8}u(?:, )?){9})\}", text.split("kAnemoiDelta")[0])]
    assert len(keys) == 56
    want = [k for r in range(14) for k in a.KEYS_X[r] + a.KEYS_Y[r]]
    assert keys == [(k << 261) % R for k in want]
    assert val(re.search(r"kAnemoiDelta\[9\] = \{([^}]*)\}", text).group(1)) == (a.DELTA << 261) % R
    assert val(re.search(r"kAnemoiG\[9\] = \{([^}]*)\}", text).group(1)) == (a.G << 261) % R
    words = re.findall(r"0x([0-9a-f]{8})u", re.search(r"kAnemoiAlphaInv\[8\] = \{([^}]*)\}", text).group(1))
    assert sum(int(w, 16) << (32 * i) for i, w in enumerate(words)) == a.ALPHA_INV
    digits = [int(d) for d in re.search(r"kAnemoiDigits\[85\] = \{([^}]*)\}", text).group(1).split(",")]
    top = int(re.search(r"kAnemoiTopDigit = (\d+)", text).group(1))
    assert len(digits) == 85 and digits[-1] == top != 0 and sum(d << (3 * i) for i, d in enumerate(digits)) == a.ALPHA_INV
    # the chain the device walks: start at t^top, then per window three squarings and a product by t^digit
    t = 0x123456789ABCDEF
    acc = pow(t, top, R)
    for d in reversed(digits[:-1]):
        acc = pow(acc, 8, R) * pow(t, d, R) % R
    assert pow(acc, 5, R) == t


EDGE_STATES = [[0, 0, 0, 0], [R - 1] * 4, [1, 0, 0, 0], [0, 0, 0, 1], [R - 1, 0, 1, R - 2]]


def test_the_inverse_undoes_the_permutation():
    rng = random.Random("anemoi-inverse")
    for s in EDGE_STATES + [[rng.randrange(R) for _ in range(4)] for _ in range(6)]:
        out = a.permute(s)
        assert out != s and a.permute_inverse(out) == s
        assert a.permute(a.permute_inverse(s)) == s


@pytest.mark.parametrize("rnd", (0, 7, 13))
def test_states_built_backwards_hit_the_chosen_root_input(rnd):
    for column in (0, 1):
        for value in (0, 1):
            s = a.state_with_sbox_input(rnd, column, value)
            assert a.sbox_inputs(s)[rnd][column] == value
            assert a.permute_inverse(a.permute(s)) == s


def _check_round_relations(tr):
    """the forward relations of test_anemoi_variable_length_hash_flatten on every round of every permutation of a trace: with (X, Y) the
    state after the keys and the linear layer,  (Y - y_after)^5 + g Y^2 = X  and  (Y - y_after)^5 + g y_after^2 + delta = x_after"""
    for before, mid, after in zip(tr.before, tr.mid, tr.after):
        prev = before
        for r in range(a.ROUNDS):
            x = [(prev[i] + a.KEYS_X[r][i]) % R for i in range(2)]
            y = [(prev[2 + i] + a.KEYS_Y[r][i]) % R for i in range(2)]
            x, y = a.linear(x, y)
            for i in range(2):
                xa, ya = mid[r][i], mid[r][2 + i]
                fifth = pow(y[i] - ya, 5, R)
                assert (fifth + a.G * y[i] * y[i]) % R == x[i]
                assert (fifth + a.G * ya * ya + a.DELTA) % R == xa
            prev = mid[r]
        x, y = a.linear(prev[:2], prev[2:])
        assert x + y == after


def test_every_round_of_a_trace_satisfies_the_forward_relations():
    tr = a.eval_variable_length_hash_with_trace([1, 2, 3, 4])
    assert len(tr.before) == 2 and tr.before[0] == [1, 2, 3, 0] and tr.output == a.golden()["hash"]
    assert tr.before[1] == [(tr.after[0][0] + 4) % R, (tr.after[0][1] + 1) % R, tr.after[0][2], tr.after[0][3]]
    _check_round_relations(tr)
    ts = a.eval_stream_cipher_with_trace([1, 2, 3], 7)               # sigma = 1, two full squeezes and a partial one
    assert len(ts.before) == 3 and len(ts.flat()) == 3 * 64
    assert ts.before[1] == ts.after[0][:3] + [(ts.after[0][3] + 1) % R] and ts.before[2] == ts.after[1]
    assert ts.output == ts.after[0][:3] + ts.after[1][:3] + ts.after[2][:1]
    _check_round_relations(ts)


def test_the_padding_table():
    want = {0: ([1, 0, 0], 0), 1: ([7, 1, 0], 0), 2: ([7, 7, 1], 0), 3: ([7, 7, 7], 1), 4: ([7, 7, 7, 7, 1, 0], 0), 5: ([7, 7, 7, 7, 7, 1], 0),
            6: ([7] * 6, 1), 7: ([7] * 7 + [1, 0], 0)}
    for n in range(8):
        assert a.pad([7] * n) == want[n]
    assert a.eval_variable_length_hash([]) == a.permute([1, 0, 0, 0])[0]
    assert a.eval_variable_length_hash([5]) == a.permute([5, 1, 0, 0])[0] != a.eval_variable_length_hash([5, 1]) != a.eval_variable_length_hash([5, 1, 0])


def test_permutation_counts_agree_with_the_library():
    from uzkge_amd import _native as N
    for length in range(9):
        for out_len in range(11):
            want = a.permutations(length, out_len)
            assert N.lib.uzk_anemoi_permutations(length, out_len) == want
            if out_len:
                assert len(a.eval_stream_cipher_with_trace([3] * length, out_len).before) == want
            else:
                assert len(a.eval_variable_length_hash_with_trace([3] * length).before) == want
    assert a.permutations(12) == 4 and a.permutations(2, 49) == 17 and a.permutations(96, 96) == 32 + 31


def test_sigma_reaches_the_squeezes():
    with_sigma, without = a.eval_stream_cipher([1, 2, 3], 4), a.eval_stream_cipher([1, 2, 3], 4, sigma_override=0)
    assert with_sigma[:3] == without[:3] and with_sigma[3] != without[3]
    assert a.eval_stream_cipher([1, 2, 3, 4], 7, sigma_override=1)[:3] == a.golden()["stream"][:3]
    assert a.eval_stream_cipher([1, 2, 3, 4], 7, sigma_override=1)[3:] != a.golden()["stream"][3:]


def test_the_reveal0_challenge_composed_with_the_curve_restatement():
    rng = random.Random("anemoi-reveal0")
    sk, omega = rng.randrange(1, e.L), rng.randrange(e.L)
    e1 = e.mul(rng.randrange(2, e.L), e.G)
    reveal, blob = a.prove0(sk, e1, omega)
    st = (*e1, *reveal, *e.keypair_public(sk))
    verdict, c = a.verify0(st, blob, want_challenge=True)
    pa, pb, _ = e.parse_proof(blob)
    assert verdict == 0 and c == a.eval_variable_length_hash([*e1, *e.G, *reveal, *st[4:6], *pa, *pb]) % e.L
    assert a.permutations(12) == 4 and a.pad(list(range(12)))[1] == 1
    assert e.verify(st, blob) in (e.EQ1_FAILS, e.EQ2_FAILS)          # the Keccak verifier rejects it, and the reverse
    assert a.verify0(st, e.prove(sk, e1, omega)[1]) in (e.EQ1_FAILS, e.EQ2_FAILS)
    bent = e.make_proof(pa, pb, (e.parse_proof(blob)[2] + 1) % e.L)
    assert a.verify0(st, bent) == e.EQ1_FAILS
    # the identity enters the hash as (0, 0) (supposed from upstream arkworks), not as (0, 1)
    assert a.point_words(e.IDENTITY) == (0, 0) and a.point_words(e.G) == e.G
    reveal, blob = a.prove0(sk, e.IDENTITY, omega)
    assert reveal == e.IDENTITY
    st = (*e.IDENTITY, *reveal, *e.keypair_public(sk))
    verdict, c = a.verify0(st, blob, want_challenge=True)
    pa, pb, _ = e.parse_proof(blob)
    assert verdict == 0 and pa == e.IDENTITY
    assert c == a.eval_variable_length_hash([0, 0, *e.G, 0, 0, *st[4:6], 0, 0, *pb]) % e.L
    assert c != a.eval_variable_length_hash([0, 1, *e.G, 0, 1, *st[4:6], 0, 1, *pb]) % e.L


def test_the_challenge_reduction_covers_the_top_of_the_field():
    assert R // e.L == 7 and 7 * e.L < R < 8 * e.L


def test_entry_points_check_their_arguments_before_the_device():
    from uzkge_amd import _native as N
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    E = N.UZK_ERR_PARAMETER
    ok = e.fr_wire([1, 2, 3, 4, 5, 6, 7, 8])
    bad = ok.copy()
    bad[5] = e.raw_wire([R])[0]                                      # r itself: the smallest word that is not below r
    out = np.zeros((128, 4), dtype=np.uint64)
    big = N.ANEMOI_MAX_BATCH + 1
    lib = N.lib
    assert lib.uzk_anemoi_permute_batch(P(ok), 0, P(out)) == E and lib.uzk_anemoi_permute_batch(P(ok), big, P(out)) == E
    assert lib.uzk_anemoi_permute_batch(None, 2, P(out)) == E and lib.uzk_anemoi_permute_batch(P(ok), 2, None) == E
    assert lib.uzk_anemoi_permute_batch(P(bad), 2, P(out)) == E
    assert lib.uzk_anemoi_hash_batch(P(ok), 4, 0, P(out), None) == E and lib.uzk_anemoi_hash_batch(P(ok), 4, big, P(out), None) == E
    assert lib.uzk_anemoi_hash_batch(P(ok), N.ANEMOI_MAX_INPUT + 1, 1, P(out), None) == E
    assert lib.uzk_anemoi_hash_batch(None, 4, 2, P(out), None) == E and lib.uzk_anemoi_hash_batch(P(ok), 4, 2, None, None) == E
    assert lib.uzk_anemoi_hash_batch(P(bad), 4, 2, P(out), None) == E and lib.uzk_anemoi_hash_batch(P(bad), 8, 1, P(out), None) == E
    assert lib.uzk_anemoi_stream_batch(P(ok), 4, 2, 0, P(out), None) == E
    assert lib.uzk_anemoi_stream_batch(P(ok), 4, 2, N.ANEMOI_MAX_OUTPUT + 1, P(out), None) == E
    assert lib.uzk_anemoi_stream_batch(P(ok), 4, 0, 3, P(out), None) == E and lib.uzk_anemoi_stream_batch(P(ok), 4, big, 3, P(out), None) == E
    assert lib.uzk_anemoi_stream_batch(P(ok), N.ANEMOI_MAX_INPUT + 1, 1, 3, P(out), None) == E
    assert lib.uzk_anemoi_stream_batch(P(bad), 2, 4, 3, P(out), None) == E and lib.uzk_anemoi_stream_batch(None, 2, 4, 3, P(out), None) == E
    assert lib.uzk_anemoi_stream_batch(P(ok), 2, 4, 3, None, None) == E
    # the zk-friendly reveals: the checks of uzk_cp_reveal_prove_batch / _verify_batch
    pts, badp = ok.reshape(4, 8), bad.reshape(4, 8)                   # four points; the third of badp has a word that is r
    sc, blob, st8 = np.zeros((4, 4), dtype=np.uint64), np.zeros(4 * N.CP_PROOF_BYTES, dtype=np.uint8), np.zeros(8, dtype=np.uint8)
    assert lib.uzk_cp_reveal_prove0_batch(P(sc), P(pts), P(sc), 0, P(out), P(out), P(blob)) == E
    assert lib.uzk_cp_reveal_prove0_batch(P(sc), P(pts), P(sc), N.CP_MAX_BATCH + 1, P(out), P(out), P(blob)) == E
    assert lib.uzk_cp_reveal_prove0_batch(P(sc), P(badp), P(sc), 4, P(out), P(out), P(blob)) == E
    assert lib.uzk_cp_reveal_prove0_batch(None, P(pts), P(sc), 1, P(out), P(out), P(blob)) == E
    assert lib.uzk_cp_reveal_prove0_batch(P(sc), P(pts), P(sc), 1, P(out), P(out), None) == E
    assert lib.uzk_cp_reveal_verify0_batch(P(pts), P(blob), 0, P(st8), None) == E
    assert lib.uzk_cp_reveal_verify0_batch(P(pts), P(blob), N.CP_MAX_BATCH + 1, P(st8), None) == E
    assert lib.uzk_cp_reveal_verify0_batch(P(pts), None, 1, P(st8), None) == E and lib.uzk_cp_reveal_verify0_batch(None, P(blob), 1, P(st8), None) == E
    assert lib.uzk_cp_reveal_verify0_batch(P(pts), P(blob), 1, None, None) == E


def test_the_python_layer_refuses_what_the_library_would():
    from uzkge_amd import anemoi as an
    with pytest.raises(ValueError):
        an.to_wire([R])
    with pytest.raises(ValueError):
        an.eval_variable_length_hash([[1, 2], [1]])
    with pytest.raises(ValueError):
        an.anemoi_permutation([[1, 2, 3]])
    assert an.from_wire(an.to_wire([0, 1, R - 1])) == [0, 1, R - 1]
