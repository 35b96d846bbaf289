"""The G1 transform (uzk_ntt_g1*, uzk_srs_to_lagrange, uzk_srs_download) on the device.  Every comparison is equality of
canonical bytes or of affine points: against the reference's own SRS files, against known discrete logs, against the product's
MSM, against the helper transform of tests/g1_ntt_ref.py, and -- at the sizes no CPU transform reaches -- through the symmetry of
the DFT matrix with the oracle's MSM on both sides."""
import os
import sys

import numpy as np
import pytest

import bn254_py as opy
import oracle_c as oc
import g1_ntt_ref as ref
from util import GOLDEN, affine_of, load_srs, rand_fr_wire

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

MAX_LOG2 = 20                      # == UZK_NTT_G1_MAX_LOG2 (tests/test_g1_ntt_host.py ties the two)
LARGE_LOG2 = (16, 18, MAX_LOG2)


def _wire(pts):
    return oc.points_from_affine(pts)


def _point(k):
    return opy.g1_mul(opy.G1_GEN, k)


@pytest.mark.parametrize("n", [4096, 8192, 16384])
def test_reference_files_exact(gpu, n):
    """forward(lagrange-srs-n) is the monomial SRS: its first 2051 points are srs-padding.bin's; the inverse returns the file's
    points; the symmetric-matrix check covers the powers the padding file does not hold."""
    lag, _ = load_srs(f"lagrange-srs-{n}.bin")
    pad, _ = load_srs("srs-padding.bin")
    mono = gpu.ntt_g1(lag)
    assert np.array_equal(mono[:2051], pad[:2051])
    assert np.array_equal(gpu.ntt_g1(mono, inverse=True), lag)
    for seed in (1, 2):
        assert ref.symmetric_ok(lag, mono, rand_fr_wire(n, 100 * n + seed))


def test_the_shipped_lagrange_file_reproduced(gpu):
    """monomial SRS -> to_lagrange -> download -> to_unchecked_bytes == lagrange-srs-4096.bin, byte for byte."""
    from uzkge_amd.poly_commit import KZGCommitmentSchemeBN254
    n = 4096
    raw = open(os.path.join(GOLDEN, f"lagrange-srs-{n}.bin"), "rb").read()
    lag, _ = load_srs(f"lagrange-srs-{n}.bin")
    pcs = KZGCommitmentSchemeBN254(gpu.ntt_g1(lag))
    lpcs = pcs.lagrange(n)
    try:
        assert lpcs.max_degree() + 1 == n
        assert lpcs.to_unchecked_bytes() == raw
    finally:
        lpcs.release(); pcs.release()


@pytest.mark.parametrize("n", [1, 2, 4, 8, 64, 512])
def test_known_tau_exact(gpu, n):
    """M[j] = [tau^j] G -> L[i] = [L_i(tau)] G with L_i(tau) = intt(powers of tau)[i]: every point, and the helper's transform."""
    tau = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543210 + n
    mono, pw = ref.tau_powers(tau, n)
    coef = oc.ntt(oc.fr_from_ints(pw), inverse=True) if n > 1 else oc.fr_from_ints(pw)
    want = np.stack([oc.g1_to_affine(oc.g1_mul(ref.G1, coef[i])) for i in range(n)])
    got = gpu.ntt_g1(mono, inverse=True)
    assert np.array_equal(got, want)
    assert np.array_equal(gpu.ntt_g1(got), mono)
    if n <= 64:
        assert np.array_equal(got, ref.g1_ntt(mono, inverse=True))
        assert np.array_equal(gpu.ntt_g1(mono), ref.g1_ntt(mono))


@pytest.mark.parametrize("n", [256, 1024])
def test_against_the_products_msm(gpu, n):
    """forward(P)[k] == msm(P, row k of the DFT matrix) for every k (rows: the Fr transform of the unit vectors)."""
    lag, _ = load_srs("lagrange-srs-4096.bin")
    pts = np.ascontiguousarray(lag[1000:1000 + n])
    fwd = gpu.ntt_g1(pts)
    one = oc.fr_from_ints([1])[0]
    srs = gpu.Srs.from_host(pts)
    try:
        for lo in range(0, n, 64):
            rows = np.zeros((64, n, 4), dtype=np.uint64)
            for r in range(64):
                e = np.zeros((n, 4), dtype=np.uint64); e[lo + r] = one
                rows[r] = oc.ntt(e)
            cms = gpu.msm_batch(srs, rows)
            for r in range(64):
                assert np.array_equal(oc.g1_to_affine(np.ascontiguousarray(cms[r])), fwd[lo + r]), lo + r
    finally:
        srs.release()


@pytest.mark.parametrize("n", [16, 4096])
def test_edge_inputs(gpu, n):
    """Infinity in the input, doubling and cancellation in every stage, infinity in the output."""
    p = _point(0xC0FFEE + n)
    pw = _wire([p])[0]
    n_p = _wire([opy.g1_mul(p, n)])[0]
    # all points equal: [n P, inf, ...] -- every first-stage butterfly doubles (A = B) and cancels (A - B)
    x = np.tile(pw, (n, 1))
    f = gpu.ntt_g1(x)
    assert np.array_equal(f[0], n_p) and not f[1:].any()
    assert np.array_equal(gpu.ntt_g1(f, inverse=True), x)
    # one point, the rest infinity: every output is that point
    x = np.zeros((n, 8), dtype=np.uint64); x[0] = pw
    f = gpu.ntt_g1(x)
    assert np.array_equal(f, np.tile(pw, (n, 1)))
    assert np.array_equal(gpu.ntt_g1(np.tile(pw, (n, 1)), inverse=True), x)
    # all infinity
    z = np.zeros((n, 8), dtype=np.uint64)
    assert not gpu.ntt_g1(z).any() and not gpu.ntt_g1(z, inverse=True).any()
    # P, -P alternating: sum_i (-w^k)^i P = n P at k = n / 2, infinity elsewhere
    x = np.tile(np.stack([pw, _wire([opy.g1_neg(p)])[0]]), (n // 2, 1))
    f = gpu.ntt_g1(x)
    assert np.array_equal(f[n // 2], n_p) and not f[:n // 2].any() and not f[n // 2 + 1:].any()
    # the reference's real shape (gen_params/mod.rs:160-173): powers, then the identity up to n
    pad, _ = load_srs("srs-padding.bin")
    live = 2051 if n == 4096 else 9
    x = np.zeros((n, 8), dtype=np.uint64); x[:live] = pad[:live]
    for inverse in (False, True):
        f = gpu.ntt_g1(x, inverse=inverse)
        if n == 16:
            assert np.array_equal(f, ref.g1_ntt(x, inverse))
        assert ref.symmetric_ok(x, f, rand_fr_wire(n, 7 + inverse), inverse)
        assert np.array_equal(gpu.ntt_g1(f, inverse=not inverse), x)


@pytest.mark.parametrize("k", LARGE_LOG2)
def test_large_whole_vector(gpu, k):
    """Random device points: in place == out of place, forward then inverse returns the input bytes, and the symmetric-matrix
    check holds for both directions with the oracle's MSM on both sides."""
    b = gpu
    n = 1 << k
    threads = min(16, os.cpu_count() or 1)
    d_in, d_out = b.dev_alloc(64 * n), b.dev_alloc(64 * n)
    try:
        b.synth_points_random(d_in, n, 0x6E7474 + k)
        b.sync()
        pts = b.dev_download(d_in, (n, 8))
        b.ntt_g1_device(d_in, d_out, n, sync=True)
        fwd = b.dev_download(d_out, (n, 8))
        assert np.array_equal(b.dev_download(d_in, (n, 8)), pts)                 # out of place leaves the input alone
        b.ntt_g1_device(d_in, d_in, n, sync=True)
        assert np.array_equal(b.dev_download(d_in, (n, 8)), fwd)
        b.ntt_g1_device(d_in, d_in, n, inverse=True, sync=True)
        assert np.array_equal(b.dev_download(d_in, (n, 8)), pts)
        b.ntt_g1_device(d_in, d_out, n, inverse=True, sync=True)
        inv = b.dev_download(d_out, (n, 8))
        assert ref.symmetric_ok(pts, fwd, rand_fr_wire(n, 31 * k), False, threads)
        assert ref.symmetric_ok(pts, inv, rand_fr_wire(n, 37 * k), True, threads)
    finally:
        b.dev_free(d_in); b.dev_free(d_out)


def test_derived_bases_serve_the_prover_at_a_shipped_size(gpu):
    """A circuit over inverse(forward(lagrange-srs-8192)) returns from round 1 the commitments of a circuit over the shipped
    bases."""
    import prover_chain as pch
    b = gpu
    n = 8192
    inp = pch.ChainInputs(n, 77)
    derived = b.ntt_g1(b.ntt_g1(inp.lagrange_wire), inverse=True)
    hiding = list(pch.HIDE_W) + [pch.HIDE_WSEL] * 3

    def round1(lagrange_wire):
        cir = b.Circuit(n, lagrange_wire, inp.bases[n:], inp.perm, inp.k, inp.anemoi_g, inp.anemoi_g_inv, inp.edwards_a,
                        [inp.table_polys[i] for i in range(pch.N_TABLES)], shuffle=True, precompute=False, synthetic=True)
        pr = b.Prover(n, 1, shared=False)
        try:
            return pr.round1(cir, inp.w_evals.reshape(1, 5 * n, 4), inp.wsel_evals.reshape(1, 3 * n, 4), np.arange(8, dtype=np.uint32),
                             inp.pi_evals[:8].reshape(1, 8, 4), hiding, np.concatenate([inp.blinds_w, inp.blinds_wsel]))
        finally:
            pr.destroy(); cir.release()

    want, got = round1(inp.lagrange_wire), round1(derived)
    assert [affine_of(j) for j in got] == [affine_of(j) for j in want]
    assert np.array_equal(derived, inp.lagrange_wire)


def test_lagrange_commit_at_a_size_the_reference_cannot_serve(gpu):
    """n = 2^15 with a known tau, independent of every shipped file: M[j] = [tau^j] G on the host, to_lagrange on the device, and
    the commit of a random evaluation vector e over the derived bases is [sum_i e_i L_i(tau)] G."""
    from uzkge_amd.poly_commit import FpPolynomial, KZGCommitmentSchemeBN254, ProverCommit
    b = gpu
    n = 1 << 15
    tau = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % opy.R
    mono, pw = ref.tau_powers(tau, n)
    pcs = KZGCommitmentSchemeBN254(mono)
    lpcs = pcs.lagrange(n)
    try:
        assert b.ntt_g1_supported(n) and lpcs.max_degree() + 1 == n
        lag_tau = oc.fr_to_ints(oc.ntt(oc.fr_from_ints(pw), inverse=True, threads=4))
        e = rand_fr_wire(n, 2015)
        s = sum(x * y for x, y in zip(oc.fr_to_ints(e), lag_tau)) % opy.R
        want = opy.g1_mul(opy.G1_GEN, s)
        assert affine_of(b.msm(lpcs._srs, e)) == want
        commit = ProverCommit(pcs, lpcs, n)
        assert commit.lagrange_pcs is lpcs
        assert affine_of(commit(e, FpPolynomial.from_coefs(np.zeros((1, 4), dtype=np.uint64)), np.zeros((0, 4), dtype=np.uint64))) == want
    finally:
        lpcs.release(); pcs.release()


def test_derived_handle_lifecycle(gpu):
    """A derived handle works from a second context on the same device, reports its length, downloads what uzk_ntt_g1 returns
    for the same input (also in part), refuses ranges past its end, and is gone after release."""
    import ctypes
    from uzkge_amd import UzkgeError, _native as N
    b = gpu
    n = 2048
    lag, _ = load_srs("lagrange-srs-4096.bin")
    mono_srs = b.Srs.from_host(lag[:3000])
    try:
        with pytest.raises(UzkgeError) as e:
            mono_srs.to_lagrange(4096)                                          # more than the handle holds
        assert e.value.kind == "DegreeError"
        d = mono_srs.to_lagrange(n)
        want = b.ntt_g1(lag[:n], inverse=True)
        ln = ctypes.c_size_t(0)
        assert N.lib.uzk_srs_len(d.handle, ctypes.byref(ln)) == N.UZK_OK and ln.value == n == d.n
        assert np.array_equal(d.download(), want)
        assert np.array_equal(d.download(5, 100), want[5:105])
        assert d.download(n, 0).shape == (0, 8)
        with pytest.raises(UzkgeError) as e:
            d.download(n - 3, 4)
        assert e.value.kind == "DegreeError"
        s = rand_fr_wire(n, 8)
        here = affine_of(b.msm(d, s))
        assert here == oc.jac_to_affine_ints(oc.msm_pippenger(want, s, 0, 4))
        h = b.ctx_create()
        try:
            b.ctx_set_current(h)
            assert affine_of(b.msm(d, s)) == here
            assert np.array_equal(d.download(0, 16), want[:16])
            d2 = mono_srs.to_lagrange(n)                                        # and derives from there too (its own plan and workspace)
            try:
                assert np.array_equal(d2.download(), want)
            finally:
                d2.release()
        finally:
            b.ctx_set_current(0)
            b.ctx_destroy(h)
        handle = d.handle
        d.release()
        assert N.lib.uzk_srs_len(handle, ctypes.byref(ln)) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_srs_release(handle) == N.UZK_ERR_PARAMETER
        out = np.zeros((1, 8), dtype=np.uint64)
        assert N.lib.uzk_srs_download(handle, 0, 1, out.ctypes.data_as(ctypes.c_void_p)) == N.UZK_ERR_PARAMETER
    finally:
        mono_srs.release()
