"""The host side of the SRS check: uzk_srs_fold_weights against the derivation restated in Python (tests/srs_check_ref.py), and the
argument errors of the validation entry points that are reported before anything touches a device."""
import ctypes

import numpy as np
import pytest

import oracle_c as oc
import srs_check_ref as ref

SEED = bytes(range(7, 39))


@pytest.mark.parametrize("first,count", [
    (0, 8), (1, 6),            # starts on an odd index: the first digest is half used
    (0, 7), (2, 5),            # ends on an even index: the last digest is half used
    (3, 9), (5, 1), (4, 1),    # odd to odd; a range of one weight, the odd and the even half of a digest
    (2 ** 33 + 1, 4), (2 ** 40, 3), (2 ** 64 - 6, 5),   # block indices >= 2^32, up to the last whole block
])
def test_fold_weights_match_the_python_derivation(first, count):
    from uzkge_amd import backend as b
    got = b.srs_fold_weights(SEED, first, count)
    want = ref.weights_ints(SEED, first, count)
    assert oc.fr_to_ints(got) == want
    assert all(w < 2 ** 128 for w in oc.fr_to_ints(got))
    assert len(set(want)) == count                           # no digest half is handed out twice


def test_fold_weights_depend_on_the_seed_and_tile():
    """A range is the same weights whatever call it comes from; another seed gives other weights."""
    from uzkge_amd import backend as b
    whole = b.srs_fold_weights(SEED, 0, 41)
    assert np.array_equal(whole[13:30], b.srs_fold_weights(SEED, 13, 17))
    assert b.srs_fold_weights(SEED, 9, 0).shape == (0, 4)
    other = b.srs_fold_weights(bytes(32), 0, 41)
    assert not (whole == other).all(axis=1).any()
    assert oc.fr_to_ints(other) == ref.weights_ints(bytes(32), 0, 41)


def test_argument_errors_need_no_device():
    from uzkge_amd import UzkgeError, _native as N, backend as b
    out = np.zeros((4, 4), dtype=np.uint64)
    pt = np.zeros(12, dtype=np.uint64)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    seed = ctypes.c_char_p(SEED)
    assert N.lib.uzk_srs_fold_weights(None, 0, 4, P(out)) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_fold_weights(seed, 0, 4, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_fold_weights(seed, 2 ** 64 - 3, 4, P(out)) == N.UZK_ERR_PARAMETER     # first + count wraps
    assert N.lib.uzk_srs_fold_weights(seed, 0, 0, None) == N.UZK_OK
    rep = N.SrsCurveReport()
    unknown = 987654321
    assert N.lib.uzk_srs_check_curve(unknown, 0, 1, ctypes.byref(rep)) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_check_curve(unknown, 0, 1, None) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_check_curve((1 << 61) | 5, 0, 1, ctypes.byref(rep)) == N.UZK_ERR_PARAMETER   # shaped like a sharded handle
    assert N.lib.uzk_srs_fold_powers(unknown, 0, 4, seed, P(pt), P(pt)) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_fold_powers(unknown, 0, 4, None, P(pt), P(pt)) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_fold_powers(unknown, 0, 4, seed, None, P(pt)) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_fold_powers(unknown, 0, 4, seed, P(pt), None) == N.UZK_ERR_PARAMETER
    for count in (0, 1):
        assert N.lib.uzk_srs_fold_powers(unknown, 0, count, seed, P(pt), P(pt)) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_fold_powers_lagrange(unknown, 4096, seed, P(pt), P(pt), P(pt)) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_fold_powers_lagrange(unknown, 4096, seed, None, P(pt), P(pt)) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_srs_fold_powers_lagrange(unknown, 3 << 10, seed, P(pt), P(pt), P(pt)) == N.UZK_ERR_FFT
    assert N.lib.uzk_srs_fold_powers_lagrange(unknown, 1, seed, P(pt), P(pt), P(pt)) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_test_srs_weights_device(None, 4, P(out)) == N.UZK_ERR_PARAMETER
    with pytest.raises(UzkgeError) as e:
        b.srs_fold_weights(b"short", 0, 1)
    assert e.value.kind == "ParameterError"


def test_the_report_struct_is_the_headers():
    from uzkge_amd import _native as N
    assert ctypes.sizeof(N.SrsCurveReport) == 40
    assert [f[0] for f in N.SrsCurveReport._fields_] == ["checked", "infinity", "non_canonical", "off_curve", "first_bad"]
