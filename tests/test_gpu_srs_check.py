"""SRS validation on the device (include/uzkge_gpu.h "SRS validation") against tests/srs_check_ref.py: the weights
of the device kernel against the host's run of the same code, the curve report point for point against Python integers, the fold
against the oracle's two MSMs under the same weights, right = tau left on power sequences with a known tau, and the verdict of the
oracle pairing over the reference's own files and its G2 pair."""
import os

import numpy as np
import pytest

import bn254_pairing as pr
import bn254_py as opy
import oracle_c as oc
import srs_check_ref as ref
from util import GOLDEN, load_srs

pytestmark = pytest.mark.gpu

SEED = bytes((37 * i + 11) & 0xFF for i in range(32))


@pytest.fixture(scope="module")
def files():
    """(lagrange-srs-4096.bin, srs-padding.bin) as wire rows, the G2 pair (H, [tau] H) of srs-padding.bin"""
    lag, _ = load_srs("lagrange-srs-4096.bin")
    pad, _ = load_srs("srs-padding.bin")
    g2 = pr.parse_srs_g2(open(os.path.join(GOLDEN, "srs-padding.bin"), "rb").read())
    return lag, pad, g2


def _int_of(row, k):
    return sum(int(row[4 * k + j]) << (64 * j) for j in range(4))


def _put(row, k, v):
    for j in range(4):
        row[4 * k + j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF


def inject(wire, i, kind):
    """the wire row i changed in place; coordinates are Montgomery words, so -y is p - y on the words too"""
    x, y = _int_of(wire[i], 0), _int_of(wire[i], 1)
    if kind == "y+1":
        _put(wire[i], 1, y + 1)
    elif kind == "x+p":                                   # >= p and still below 2^256 (p < 2^254)
        _put(wire[i], 0, x + opy.P)
    elif kind == "neg":                                   # (x, -y): a curve point, must not be reported
        _put(wire[i], 1, opy.P - y)
    elif kind == "inf":
        wire[i] = 0
    elif kind == "zero_x":                                # (0, y)
        _put(wire[i], 0, 0)
    else:
        raise AssertionError(kind)


KINDS = ("y+1", "x+p", "neg", "inf", "zero_x")


def _report_matches(b, wire, offset=0, count=None):
    srs = b.Srs.from_host(wire)
    try:
        got = srs.check_curve(offset, count)
    finally:
        srs.release()
    want = ref.curve_report(wire, offset, count)
    assert got == want, (got, want)
    return got


# ---- 1. weights -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [2, 3, 64, 65, 129, 4099])
def test_device_weights_equal_the_host_function(gpu, count):
    """odd counts use half of the last digest; 129 weights are 65 digests, one past a wave; 4099 several workgroups"""
    dev = gpu.srs_fold_weights_device(SEED, count)
    assert np.array_equal(dev, gpu.srs_fold_weights(SEED, 0, count))
    assert oc.fr_to_ints(dev[:5]) == ref.weights_ints(SEED, 0, min(count, 5))


# ---- 2. curve report ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_curve_report_point_for_point(gpu, files, n):
    lag, pad, _ = files
    base = np.concatenate([lag, pad])[:n].copy()
    clean = _report_matches(gpu, base)
    assert clean == {"checked": n, "infinity": 0, "non_canonical": 0, "off_curve": 0, "first_bad": None}
    # index 0, the last point, the last lane of a wave and of a workgroup, one in the middle
    spots = sorted({i for i in (0, n - 1, 63, 255, n // 2, 64, 256) if i < n})
    for k, kind in enumerate(KINDS):                      # singly, each kind
        w = base.copy()
        at = spots[k % len(spots)]
        inject(w, at, kind)
        rep = _report_matches(gpu, w)
        assert rep["first_bad"] == (at if kind in ("y+1", "x+p", "zero_x") else None), (kind, at, rep)
    for at in spots:                                      # a bad point at every spot, singly
        w = base.copy()
        inject(w, at, "y+1")
        rep = _report_matches(gpu, w)
        assert rep["first_bad"] == at and rep["off_curve"] == 1
    together = (spots[::-1] + [i for i in range(1, 6) if i < n and i not in spots])[:len(KINDS)]
    if len(together) == len(KINDS):                       # together: one of each kind (n >= 5)
        w = base.copy()
        for at, kind in zip(together, KINDS):
            inject(w, at, kind)
        rep = _report_matches(gpu, w)
        assert (rep["infinity"], rep["non_canonical"], rep["off_curve"]) == (1, 1, 2)
        good = sum(ref.classify(r) == "good" for r in w)
        assert rep["infinity"] + rep["non_canonical"] + rep["off_curve"] + good == rep["checked"] == n


def test_curve_report_first_bad_across_workgroups_and_offsets(gpu, files):
    lag, pad, _ = files
    w = np.concatenate([lag, pad])[:4099].copy()
    inject(w, 3000, "x+p")
    inject(w, 300, "y+1")
    inject(w, 5, "zero_x")
    srs = gpu.Srs.from_host(w)
    try:
        assert srs.check_curve() == ref.curve_report(w) and srs.check_curve()["first_bad"] == 5
        rep = srs.check_curve(6)                          # the bad point below the run is not looked at
        assert rep == ref.curve_report(w, 6) and rep["first_bad"] == 300 and rep["checked"] == 4093
        rep = srs.check_curve(301)
        assert rep == ref.curve_report(w, 301) and rep["first_bad"] == 3000 and (rep["non_canonical"], rep["off_curve"]) == (1, 0)
        assert srs.check_curve(6, 294)["first_bad"] is None and srs.check_curve(6, 295)["first_bad"] == 300
        assert srs.check_curve(3000, 1) == {"checked": 1, "infinity": 0, "non_canonical": 1, "off_curve": 0, "first_bad": 3000}
        assert srs.check_curve(4099, 0) == {"checked": 0, "infinity": 0, "non_canonical": 0, "off_curve": 0, "first_bad": None}
    finally:
        srs.release()


def test_curve_report_when_a_workgroup_takes_several_rounds(gpu, files):
    """Beyond num_cus * 8 workgroups of 256 lanes (2^19 points on 256 compute units) a lane strides over several points.  The
    bases are the 4096 points of the Lagrange file over and over (all good: the point-for-point test), so the expected report
    follows from the injected rows alone."""
    lag, _, _ = files
    n = (1 << 19) + (1 << 18) + 3
    w = np.tile(lag, (n // 4096 + 1, 1))[:n].copy()
    srs = gpu.Srs.from_host(w)
    try:
        assert srs.check_curve() == {"checked": n, "infinity": 0, "non_canonical": 0, "off_curve": 0, "first_bad": None}
    finally:
        srs.release()
    # a wave's second-round hit, then an earlier index of another workgroup, then the wave's own first round
    plan = [((1 << 19) + 3, "y+1"), (n - 1, "x+p"), (300000, "zero_x"), (10, "y+1"), (n - 2, "inf"), (7, "neg")]
    want = {"checked": n, "infinity": 0, "non_canonical": 0, "off_curve": 0, "first_bad": None}
    for at, kind in plan:
        inject(w, at, kind)
        c = ref.classify(w[at])
        if c != "good":
            want[c] += 1
        if c in ("non_canonical", "off_curve"):
            want["first_bad"] = at if want["first_bad"] is None else min(want["first_bad"], at)
        srs = gpu.Srs.from_host(w)
        try:
            assert srs.check_curve() == want, (at, kind)
        finally:
            srs.release()
    assert want["first_bad"] == 10 and (want["infinity"], want["non_canonical"], want["off_curve"]) == (1, 1, 3)


# ---- 3. the fold against the oracle's two MSMs ------------------------------------------------------------------------------------
def _fold_matches(b, srs, wire, offset, count, seed=SEED):
    left, right = srs.fold_powers(seed, offset, count)
    want_l, want_r = ref.fold(wire, seed, offset, count)
    assert ref.affine_wire(left).tobytes() == want_l.tobytes(), (offset, count, "left")
    assert ref.affine_wire(right).tobytes() == want_r.tobytes(), (offset, count, "right")


def test_fold_equals_the_oracle_msms(gpu, files):
    _, pad, _ = files
    srs = gpu.Srs.from_host(pad)
    try:
        for count in (2, 3, 64, 65, 2051):
            _fold_matches(gpu, srs, pad, 0, count)
        _fold_matches(gpu, srs, pad, 7, 100)                               # offset > 0
        _fold_matches(gpu, srs, pad, pad.shape[0] - 50, 50)               # ends at the handle's last point
        _fold_matches(gpu, srs, pad, 0, pad.shape[0])
    finally:
        srs.release()


def test_fold_with_infinities_in_the_run(gpu, files):
    _, pad, _ = files
    w = pad[:300].copy()
    for at in (0, 1, 63, 64, 150, 298, 299):
        w[at] = 0
    srs = gpu.Srs.from_host(w)
    try:
        assert srs.check_curve()["infinity"] == 7 and srs.check_curve()["first_bad"] is None
        _fold_matches(gpu, srs, w, 0, 300)
        _fold_matches(gpu, srs, w, 0, 2)                                   # nothing but infinities on the left
        left, right = srs.fold_powers(SEED, 0, 2)
        assert not ref.affine_wire(left).any() and not ref.affine_wire(right).any()
    finally:
        srs.release()


def test_fold_at_the_first_size_of_the_general_pipeline(gpu):
    """2^15 + 3 random points (no SRS: the comparison is the two MSMs): 2^15 + 2 weights, past the one-workgroup-per-slot pipeline"""
    import torch
    n = (1 << 15) + 3
    pts = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    gpu.synth_points_random(pts.data_ptr(), n, 20261)
    gpu.sync()
    srs = gpu.Srs.from_device(pts.data_ptr(), n)
    try:
        wire = srs.download()
        assert srs.check_curve() == {"checked": n, "infinity": 0, "non_canonical": 0, "off_curve": 0, "first_bad": None}
        _fold_matches(gpu, srs, wire, 0, n)
    finally:
        srs.release()
        del pts


# ---- 4. closed form ---------------------------------------------------------------------------------------------------------------
def test_right_is_tau_times_left_on_a_power_sequence(gpu):
    tau = 0x2A7F3C5D9E1B486072D5F0A3B6C9E2F41D3A5B7C9E0F1A2B3C4D5E6F708192A3 % opy.R
    powers, _ = ref.tau_powers(tau, 512)
    tau_wire = oc.fr_from_ints([tau])[0]
    srs = gpu.Srs.from_host(powers)
    try:
        for n in (2, 3, 65, 512):
            left, right = srs.fold_powers(SEED, 0, n)
            assert ref.affine_wire(right).tobytes() == oc.g1_to_affine(oc.g1_mul(ref.affine_wire(left), tau_wire)).tobytes(), n
        left, right = srs.fold_powers(SEED, 100, 65)                       # a run that starts at tau^100 is one too
        assert ref.affine_wire(right).tobytes() == oc.g1_to_affine(oc.g1_mul(ref.affine_wire(left), tau_wire)).tobytes()
    finally:
        srs.release()


# ---- 5. the verdict of the oracle pairing -------------------------------------------------------------------------------------------
def _verdict(b, wire, g2, count=None):
    """(curve report, accepted?) of wire[0 .. count)"""
    srs = b.Srs.from_host(wire)
    try:
        rep = srs.check_curve(0, count)
        left, right = srs.fold_powers(SEED, 0, count)
    finally:
        srs.release()
    return rep, ref.pairing_accepts(left, right, g2)


def test_the_reference_powers_are_accepted(gpu, files):
    _, pad, g2 = files
    rep, ok = _verdict(gpu, pad, g2, 2051)
    assert ok and rep == {"checked": 2051, "infinity": 0, "non_canonical": 0, "off_curve": 0, "first_bad": None}
    assert opy.wire_to_affine(pad[0].tobytes()) == opy.G1_GEN


def _double(row):
    return oc.points_from_affine([opy.g1_add(opy.wire_to_affine(row.tobytes()), opy.wire_to_affine(row.tobytes()))])[0]


@pytest.mark.parametrize("case", ["swap", "double", "negate", "first", "last", "padding"])
def test_a_run_that_is_no_power_sequence_is_rejected(gpu, files, case):
    _, pad, g2 = files
    w = pad[:2051].copy()
    count = 2051
    if case == "swap":
        w[[700, 1300]] = w[[1300, 700]]
    elif case == "double":
        w[1025] = _double(w[1025])
    elif case == "negate":
        inject(w, 64, "neg")
    elif case == "first":
        w[0] = pad[5]
    elif case == "last":
        w[2050] = pad[3]
    else:                                                                  # across the file's padding powers tau^4096 ..
        w, count = pad[:2054].copy(), 2054
    rep, ok = _verdict(gpu, w, g2, count)
    assert rep == {"checked": count, "infinity": 0, "non_canonical": 0, "off_curve": 0, "first_bad": None}
    assert not ok


# ---- 6. Lagrange ------------------------------------------------------------------------------------------------------------------
def test_lagrange_bases_through_their_forward_transform(gpu, files):
    lag, _, g2 = files
    from uzkge_amd import UzkgeError
    srs = gpu.Srs.from_host(lag)
    try:
        first, left, right = srs.fold_powers_lagrange(SEED, 4096)
        assert opy.wire_to_affine(first.tobytes()) == opy.G1_GEN
        assert ref.pairing_accepts(left, right, g2)
        with pytest.raises(UzkgeError) as e:
            srs.fold_powers_lagrange(SEED, 8192)                           # more than the handle holds
        assert e.value.kind == "DegreeError"
        with pytest.raises(UzkgeError) as e:
            srs.fold_powers_lagrange(SEED, 3 << 10)
        assert e.value.kind == "FFTError"
    finally:
        srs.release()
    w = lag.copy()
    w[[17, 2900]] = w[[2900, 17]]
    srs = gpu.Srs.from_host(w)
    try:
        assert srs.check_curve()["first_bad"] is None
        first, left, right = srs.fold_powers_lagrange(SEED, 4096)
        assert opy.wire_to_affine(first.tobytes()) == opy.G1_GEN           # the sum does not see a swap: the fold does
        assert not ref.pairing_accepts(left, right, g2)
    finally:
        srs.release()


# ---- 7. determinism, error codes, the scheme's check ----------------------------------------------------------------------------------
def test_determinism_and_error_codes(gpu, files):
    import ctypes
    from uzkge_amd import UzkgeError, _native as N
    _, pad, _ = files
    srs = gpu.Srs.from_host(pad)
    try:
        a, b2 = srs.fold_powers(SEED, 0, 500), srs.fold_powers(SEED, 0, 500)
        assert ref.affine_wire(a[0]).tobytes() == ref.affine_wire(b2[0]).tobytes() and ref.affine_wire(a[1]).tobytes() == ref.affine_wire(b2[1]).tobytes()
        other = srs.fold_powers(bytes(32), 0, 500)
        assert ref.affine_wire(other[0]).tobytes() != ref.affine_wire(a[0]).tobytes()
        for call, kind in ((lambda: srs.fold_powers(SEED, 0, 1), "ParameterError"), (lambda: srs.fold_powers(SEED, 5, 0), "ParameterError"),
                           (lambda: srs.fold_powers(SEED, 0, pad.shape[0] + 1), "DegreeError"), (lambda: srs.fold_powers(SEED, pad.shape[0], 2), "DegreeError"),
                           (lambda: srs.check_curve(1, pad.shape[0]), "DegreeError"), (lambda: srs.check_curve(pad.shape[0] + 1, 0), "DegreeError"),
                           (lambda: srs.fold_powers_lagrange(SEED, 4096), "DegreeError"), (lambda: srs.fold_powers_lagrange(SEED, 1), "ParameterError"),
                           (lambda: srs.fold_powers(b"short", 0, 4), "ParameterError")):
            with pytest.raises(UzkgeError) as e:
                call()
            assert e.value.kind == kind
        pt = np.zeros(12, dtype=np.uint64)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        assert N.lib.uzk_srs_check_curve(srs.handle, 0, 4, None) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_srs_fold_powers(srs.handle, 0, 4, None, vp(pt), vp(pt)) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_srs_fold_powers(srs.handle, 0, 4, ctypes.c_char_p(SEED), None, vp(pt)) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_srs_fold_powers_lagrange(srs.handle, 1024, ctypes.c_char_p(SEED), None, vp(pt), vp(pt)) == N.UZK_ERR_PARAMETER
        rep = N.SrsCurveReport()
        assert N.lib.uzk_srs_check_curve(srs.handle + 1000, 0, 4, ctypes.byref(rep)) == N.UZK_ERR_PARAMETER      # unknown handle
    finally:
        srs.release()
    sh = gpu.ShardedSrs(pad[:64], [0])                                     # a sharded handle is not accepted
    try:
        rep = N.SrsCurveReport()
        pt = np.zeros(12, dtype=np.uint64)
        assert N.lib.uzk_srs_check_curve(sh.handle, 0, 4, ctypes.byref(rep)) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_srs_fold_powers(sh.handle, 0, 4, ctypes.c_char_p(SEED), pt.ctypes.data_as(ctypes.c_void_p), pt.ctypes.data_as(ctypes.c_void_p)) == N.UZK_ERR_PARAMETER
    finally:
        sh.release()
    if gpu.device_count() > 1:                                             # a handle of another device
        ctx = gpu.ctx_create_on(1)
        gpu.ctx_set_current(ctx)
        try:
            far = gpu.Srs.from_host(pad[:64])
        finally:
            gpu.ctx_set_current(0)
        try:
            with pytest.raises(UzkgeError) as e:
                far.check_curve()
            assert e.value.kind == "ParameterError"
            with pytest.raises(UzkgeError) as e:
                far.fold_powers(SEED)
            assert e.value.kind == "ParameterError"
        finally:
            gpu.ctx_set_current(ctx)
            far.release()
            gpu.ctx_set_current(0)
            gpu.ctx_destroy(ctx)


def test_the_commitment_scheme_checks_itself(gpu, files):
    from uzkge_amd import UzkgeError
    from uzkge_amd.poly_commit import KZGCommitmentSchemeBN254
    _, pad, g2 = files
    pcs = KZGCommitmentSchemeBN254(pad[:2051])
    try:
        rep, left, right = pcs.check(SEED)
        assert rep["checked"] == 2051 and rep["first_bad"] is None and ref.pairing_accepts(left, right, g2)
        want_l, want_r = ref.fold(pad, SEED, 0, 2051)
        assert ref.affine_wire(left).tobytes() == want_l.tobytes() and ref.affine_wire(right).tobytes() == want_r.tobytes()
        _, l1, _ = pcs.check(offset=10, count=40)                           # the seed is drawn inside: two calls, two folds
        _, l2, _ = pcs.check(offset=10, count=40)
        assert ref.affine_wire(l1).tobytes() != ref.affine_wire(l2).tobytes()
    finally:
        pcs.release()
    w = pad[:100].copy()
    inject(w, 41, "y+1")
    bad = KZGCommitmentSchemeBN254(w)
    try:
        with pytest.raises(UzkgeError) as e:
            bad.check(SEED)
        assert e.value.kind == "ParameterError" and "41" in str(e.value)
        rep, _, _ = bad.check(SEED, 42)                                    # the run above the bad point is fine
        assert rep["first_bad"] is None
    finally:
        bad.release()
