"""GPU: Anemoi-Jive -- uzk_anemoi_permute_batch, uzk_anemoi_hash_batch, uzk_anemoi_stream_batch and the Python layer over them -- bit for
bit against tests/anemoi_ref.py: the reference's recorded answers, states built with the inverse permutation so that a chosen round's
fifth root is taken of exactly 0 or 1, every padding case, sigma reaching the squeezes, and every element of the traces.

The restatement is evaluated once per DISTINCT input; the lanes of a batch cycle through a handful of inputs (lanes 0, 63 and 64 get
different ones), since what a larger batch adds is the lane index, not the data."""
import ctypes
import functools
import random

import numpy as np
import pytest

import anemoi_ref as a

pytestmark = pytest.mark.gpu
R = a.R
DISTINCT = 5                                                         # lanes 0, 63, 64 -> inputs 0, 3, 4


@functools.lru_cache(maxsize=None)
def _permuted(state):
    return tuple(a.permute(list(state)))


@functools.lru_cache(maxsize=None)
def _pool():
    """states every batch is filled from: the edges, then random ones -- made once, never changed"""
    rng = random.Random("gpu-anemoi-states")
    edge = [(0, 0, 0, 0), (R - 1,) * 4, (0, R - 1, 1, R - 2)]
    return tuple(edge + [tuple(rng.randrange(R) for _ in range(4)) for _ in range(4)])


@functools.lru_cache(maxsize=None)
def _inputs(length):
    """DISTINCT inputs of one length; the first of length 4 is the reference's recorded case"""
    rng = random.Random("gpu-anemoi-inputs-%d" % length)
    rows = [tuple(rng.randrange(R) for _ in range(length)) for _ in range(DISTINCT)]
    if length == 4:
        rows[0] = (1, 2, 3, 4)
    if length >= 1:
        rows[1] = (R - 1,) * length
        rows[2] = (0,) * length
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _hash_trace(row):
    return a.eval_variable_length_hash_with_trace(list(row))


@functools.lru_cache(maxsize=None)
def _stream_trace(row, out_len):
    return a.eval_stream_cipher_with_trace(list(row), out_len)


def _states_wire(states):
    return a.wire([v for s in states for v in s]).reshape(len(states), 4, 4)


def _lanes(length, n):
    rows = _inputs(length)
    picked = [rows[i % DISTINCT] if length else () for i in range(n)]
    wire = a.wire([v for row in picked for v in row]).reshape(n, length, 4)
    return picked, wire


@pytest.mark.parametrize("n", (1, 63, 64, 65, 129))
def test_permute_batches(gpu, n):
    pool = _pool()
    states = [pool[(i + n) % len(pool)] for i in range(n)]
    states[0] = pool[0]                                              # zero in every word
    states[-1] = pool[1]                                             # r - 1 in every word
    got = a.unwire(gpu.anemoi_permute_batch(_states_wire(states)))
    assert [tuple(got[4 * i:4 * i + 4]) for i in range(n)] == [_permuted(s) for s in states]


@pytest.mark.parametrize("column", (0, 1))
@pytest.mark.parametrize("rnd", (0, 7, 13))
def test_roots_of_zero_and_one_at_lanes_0_63_64(gpu, rnd, column):
    """States built WITH THE INVERSE PERMUTATION so that round `rnd` takes the fifth root of exactly 0 or 1 in `column`: the values where
    an exponentiation chain most plausibly goes wrong, which random data never reaches."""
    pool = _pool()
    special = [tuple(a.state_with_sbox_input(rnd, column, v)) for v in (0, 1)]
    assert [a.sbox_inputs(list(s))[rnd][column] for s in special] == [0, 1]
    for turn in (0, 1):
        states = [pool[i % len(pool)] for i in range(65)]
        for slot, lane in enumerate((0, 63, 64)):
            states[lane] = special[(slot + turn) % 2]
        got = a.unwire(gpu.anemoi_permute_batch(_states_wire(states)))
        assert [tuple(got[4 * i:4 * i + 4]) for i in range(65)] == [_permuted(s) for s in states]


def test_both_columns_take_the_root_of_zero_at_once(gpu):
    other = (0x1234567, 0x7654321, 0)
    s = tuple(a.state_with_sbox_input(7, 0, 0, other=other))
    assert a.sbox_inputs(list(s))[7] == [0, 0]
    got = a.unwire(gpu.anemoi_permute_batch(_states_wire([s, s])))
    assert tuple(got[:4]) == tuple(got[4:]) == _permuted(s)


@pytest.mark.parametrize("length", (0, 1, 2, 3, 4, 6, 12, 96))
def test_hashes(gpu, length):
    n = 2 if length == 96 else 65
    picked, wire = _lanes(length, n)
    got = a.unwire(gpu.anemoi_hash_batch(wire, length))
    assert got == [_hash_trace(row).output for row in picked]
    assert gpu.anemoi_permutations(length) == a.permutations(length) == len(_hash_trace(picked[0]).before)
    if length == 4:
        assert got[0] == a.golden()["hash"]


@pytest.mark.parametrize("length,out_len", ((4, 2), (4, 4), (4, 6), (4, 7), (3, 4), (3, 8), (2, 49), (1, 96)))
def test_stream_cipher(gpu, length, out_len):
    picked, wire = _lanes(length, 65)
    got = a.unwire(gpu.anemoi_stream_batch(wire, out_len, length))
    want = [v for row in picked for v in _stream_trace(row, out_len).output]
    assert got == want
    assert gpu.anemoi_permutations(length, out_len) == a.permutations(length, out_len)
    if length == 4:
        assert got[:out_len] == a.golden()["stream"][:out_len]
    if length == 3:                                                  # sigma = 1 is seen by the later permutations
        assert got[3:out_len] != a.eval_stream_cipher(list(picked[0]), out_len, sigma_override=0)[3:]


def test_every_element_of_the_hash_trace(gpu):
    picked, wire = _lanes(1, 65)
    plain = gpu.anemoi_hash_batch(wire, 1)
    out, tr = gpu.anemoi_hash_batch(wire, 1, want_trace=True)
    assert np.array_equal(out, plain) and tr.shape == (65, 1, 64, 4)
    assert a.unwire(tr) == [v for row in picked for v in _hash_trace(row).flat()]


def test_every_element_of_the_stream_cipher_trace(gpu):
    picked, wire = _lanes(2, 65)
    plain = gpu.anemoi_stream_batch(wire, 49, 2)
    out, tr = gpu.anemoi_stream_batch(wire, 49, 2, want_trace=True)
    assert np.array_equal(out, plain) and tr.shape == (65, 17, 64, 4)
    assert a.unwire(tr) == [v for row in picked for v in _stream_trace(row, 49).flat()]


def test_the_python_layer_returns_the_reference_traces_fields(gpu):
    from uzkge_amd import anemoi as an
    g = a.golden()
    assert an.eval_variable_length_hash([g["input"]]) == [g["hash"]]
    assert an.eval_stream_cipher([g["input"], g["input"]], 7) == [g["stream"], g["stream"]]
    assert an.anemoi_permutation([[1, 2, 3, 4]]) == [list(_permuted((1, 2, 3, 4)))]
    assert an.eval_variable_length_hash([[]]) == [a.eval_variable_length_hash([])]
    want = _stream_trace(tuple(g["input"]), 7)
    tr = an.eval_stream_cipher_with_trace([g["input"]], 7)[0]
    assert tr["input"] == g["input"] and tr["output"] == g["stream"]
    assert tr["before_permutation"] == [(b[:2], b[2:]) for b in want.before]
    assert tr["after_permutation"] == [(b[:2], b[2:]) for b in want.after]
    assert tr["intermediate_values_before_constant_additions"] == [([m[:2] for m in mid], [m[2:] for m in mid]) for mid in want.mid]
    th = an.eval_variable_length_hash_with_trace([g["input"]])[0]
    assert th["output"] == g["hash"] and th["before_permutation"] == tr["before_permutation"][:2]


def test_refusals_leave_the_library_working(gpu):
    from uzkge_amd import _native as N
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    E = N.UZK_ERR_PARAMETER
    ok = a.wire([1, 2, 3, 4])
    bad = ok.copy()
    bad[2, 3] = np.uint64(0xFFFFFFFFFFFFFFFF)                        # a non-canonical word
    out = np.zeros((128, 4), dtype=np.uint64)
    assert N.lib.uzk_anemoi_hash_batch(P(bad), 4, 1, P(out), None) == E
    assert N.lib.uzk_anemoi_permute_batch(P(bad), 1, P(out)) == E
    assert N.lib.uzk_anemoi_hash_batch(P(ok), 4, 0, P(out), None) == E
    assert N.lib.uzk_anemoi_hash_batch(P(ok), 97, 1, P(out), None) == E
    assert N.lib.uzk_anemoi_stream_batch(P(ok), 4, 1, 0, P(out), None) == E
    assert not out.any()
    assert a.unwire(gpu.anemoi_hash_batch(ok.reshape(1, 4, 4))) == [a.golden()["hash"]]
