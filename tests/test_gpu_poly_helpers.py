"""Device polynomial helpers next to the hot path against CPU restatements of
FpPolynomial::eval (field_polynomial.rs:198-209) and z_poly (plonk/helpers.rs:160-220).
Parity here is restatement-vs-restatement plus protocol properties: the reference holds no fixture
for these intermediate values (noted as "parity unpinned" for this row in DESIGN.md)."""
import numpy as np
import pytest

import bn254_py as opy
import oracle_c as oc
from util import rand_fr, rand_fr_wire

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,batch", [(1, 1), (3, 2), (17, 5), (1024, 2), (1025, 2), (4096, 3), (16384, 9), (16387, 20), (65536, 3), (65537, 2),
                                     (98304, 6), (100000, 2), (262144, 1), (262145, 2)])
def test_poly_eval_batch(gpu, n, batch):
    """Both evaluation paths -- the one-launch kernel for <= 256 blocks of 1024 coefficients (n <= 2^18) and the table-driven one
    beyond -- against the oracle; repeated calls (the one-launch kernel's arrival counters must come back to zero)."""
    c = rand_fr_wire(n * batch, 10 + n).reshape(batch, n, 4)
    x = rand_fr_wire(1, 77)[0]
    want = [oc.poly_eval(c[b], x) for b in range(batch)]
    for rep in range(3):
        got = gpu.poly_eval_batch(c, x)
        for b in range(batch):
            assert np.array_equal(got[b], want[b]), (n, b, rep)


def test_poly_eval_special_points(gpu):
    c = rand_fr_wire(1000, 5).reshape(1, 1000, 4)
    zero = np.zeros(4, dtype=np.uint64)
    one = oc.fr_from_ints([1])[0]
    assert np.array_equal(gpu.poly_eval_batch(c, zero)[0], c[0, 0])            # p(0) = c_0
    total = c[0, 0]
    for j in range(1, 1000):
        total = oc.fr_add(total, c[0, j])
    assert np.array_equal(gpu.poly_eval_batch(c, one)[0], total)               # p(1) = sum c_j


def _domain(n):
    w = opy.root_of_unity(n)
    g, x = [], 1
    for _ in range(n):
        g.append(x)
        x = x * w % opy.R
    return oc.fr_from_ints(g)


@pytest.mark.parametrize("n,n_wires", [(2, 3), (8, 5), (1024, 5), (16384, 5), (5000, 3)])
def test_z_poly_matches_restatement(gpu, n, n_wires):
    rng = np.random.default_rng(n)
    w = rand_fr_wire(n * n_wires, 3 + n).reshape(n_wires, n, 4)
    perm = rng.integers(0, n * n_wires, size=(n_wires, n), dtype=np.uint32)
    group = _domain(n) if (n & (n - 1)) == 0 else rand_fr_wire(n, 4)
    k = oc.fr_from_ints([1, 7, 13, 17, 23][:n_wires])
    beta, gamma = rand_fr_wire(2, 99)
    got = gpu.z_poly(w, perm, group, k, beta, gamma)
    assert np.array_equal(got, oc.z_poly(w, perm, group, k, beta, gamma))
    assert oc.fr_to_ints(got[:1]) == [1]


def test_z_poly_device_entry_point(gpu):
    """uzk_z_poly_device on device-resident inputs gives the same bytes as the host-pointer entry point."""
    import torch
    n, n_wires = 5000, 5
    rng = np.random.default_rng(7)
    w = rand_fr_wire(n * n_wires, 31).reshape(n_wires, n, 4)
    perm = rng.integers(0, n * n_wires, size=(n_wires, n), dtype=np.uint32)
    group = rand_fr_wire(n, 32)
    k = oc.fr_from_ints([1, 7, 13, 17, 23])
    beta, gamma = rand_fr_wire(2, 33)
    dw = torch.from_numpy(w.view(np.int64)).to("cuda")
    dp = torch.from_numpy(perm.view(np.int32)).to("cuda")
    dg = torch.from_numpy(group.view(np.int64)).to("cuda")
    dz = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    gpu.z_poly_device(dw.data_ptr(), dp.data_ptr(), dg.data_ptr(), k, beta, gamma, n, n_wires, dz.data_ptr())
    gpu.sync()
    assert np.array_equal(dz.cpu().numpy().view(np.uint64), oc.z_poly(w, perm, group, k, beta, gamma))


def test_z_poly_closes_for_a_satisfied_permutation(gpu):
    """Protocol property: when the wire values respect the copy constraints (w at position p equals
    w at perm[p]), the grand product over the WHOLE domain is 1, i.e. z[n-1] times the last row's
    numerator/denominator equals 1 -- the identity the verifier relies on."""
    n, n_wires = 256, 5
    rng = np.random.default_rng(1)
    total = n * n_wires
    perm_flat = rng.permutation(total).astype(np.uint32)           # a genuine permutation of wire slots
    # values constant on every cycle of the permutation
    vals = [None] * total
    ints = rand_fr(total, 11)
    for start in range(total):
        if vals[start] is None:
            p = start
            while vals[p] is None:
                vals[p] = ints[start]
                p = int(perm_flat[p])
    w = oc.fr_from_ints(vals).reshape(n_wires, n, 4)
    perm = perm_flat.reshape(n_wires, n)
    group = _domain(n)
    kints = [1, 7, 13, 17, 23]
    k = oc.fr_from_ints(kints)
    b_i, g_i = rand_fr(2, 5)
    z = gpu.z_poly(w, perm, group, k, oc.fr_from_ints([b_i])[0], oc.fr_from_ints([g_i])[0])
    zl = oc.fr_to_ints(z[n - 1:n])[0]
    gi = oc.fr_to_ints(group)
    i = n - 1
    num = den = 1
    for j in range(n_wires):
        f = vals[j * n + i]
        num = num * (f + g_i + b_i * kints[j] * gi[i]) % opy.R
        pv = int(perm[j, i])
        den = den * (f + g_i + b_i * kints[pv // n] * gi[pv % n]) % opy.R
    assert zl * num % opy.R == den % opy.R


# ---- z_poly at its size classes --------------------------------------------------------------------------------------------------
# One launch (fr_scan_mul2: blocks of 2048 elements, the padded scan has n elements) up to n = 65537, the two-level scans
# (fr_scan_mul over n - 1 elements) from 65538 on.  2049: the padding element alone in the second block; 65536 / 65537: 32 / 33
# blocks, the last sizes of the one-launch path; 3 * 2^16 + 5: 97 blocks of the two-level path.
Z_SIZES = [1, 2, 3, 2047, 2048, 2049, 2050, 4097, 65536, 65537, 65538, 131073, 3 * (1 << 16) + 5]
Z_KS = [1, 7, 13, 17, 23, 29, 31, 37]                      # eight distinct coset representatives
_z_cache = {}


def _z_inputs(n, n_wires):
    """Inputs and the oracle's z of one shape, computed once per session and never written to."""
    if (n, n_wires) not in _z_cache:
        rng = np.random.default_rng(1000 * n_wires + n)
        w = rand_fr_wire(n * n_wires, 3 + n + n_wires).reshape(n_wires, n, 4)
        perm = rng.integers(0, n * n_wires, size=(n_wires, n), dtype=np.uint32)
        group = _domain(n) if (n & (n - 1)) == 0 else rand_fr_wire(n, 4 + n)
        k = oc.fr_from_ints(Z_KS[:n_wires])
        beta, gamma = rand_fr_wire(2, 99 + n)
        args = (w, perm, group, k, beta, gamma)
        for a in (w, perm, group):
            a.setflags(write=False)
        _z_cache[(n, n_wires)] = (args, oc.z_poly(*args))
    return _z_cache[(n, n_wires)]


@pytest.mark.parametrize("n,n_wires", [(n, 5) for n in Z_SIZES] + [(2049, 1), (2049, 8), (65538, 1), (65538, 8)])
def test_z_poly_at_every_size_class_and_wire_count(gpu, n, n_wires):
    """uzk_z_poly against the oracle, byte for byte.  Every case from 2047 on runs twice with a small size in between: the
    workspaces of the scans (poly_tmp, poly_tmp2, zpoly_tmp) are reused across calls and sizes."""
    args, want = _z_inputs(n, n_wires)
    got = gpu.z_poly(*args)
    assert got.shape == want.shape and np.array_equal(got, want), (n, n_wires, "first call")
    if n >= 2047:
        small, small_want = _z_inputs(3, 5)
        assert np.array_equal(gpu.z_poly(*small), small_want)
        assert np.array_equal(gpu.z_poly(*args), want), (n, n_wires, "second call")


def test_z_poly_device_entry_point_through_the_two_level_scans(gpu):
    """uzk_z_poly_device at n = 65538 (the first size of fr_scan_mul) on device-resident inputs."""
    import torch
    n, n_wires = 65538, 5
    (w, perm, group, k, beta, gamma), want = _z_inputs(n, n_wires)
    dw = torch.from_numpy(w.view(np.int64).copy()).to("cuda")
    dp = torch.from_numpy(perm.view(np.int32).copy()).to("cuda")
    dg = torch.from_numpy(group.view(np.int64).copy()).to("cuda")
    dz = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    gpu.z_poly_device(dw.data_ptr(), dp.data_ptr(), dg.data_ptr(), k, beta, gamma, n, n_wires, dz.data_ptr())
    gpu.sync()
    assert np.array_equal(dz.cpu().numpy().view(np.uint64), want)


def test_z_poly_refuses_a_permutation_value_out_of_range(gpu):
    """The kernel indexes k[perm / n] (an array of eight) and group[perm % n] unchecked; the host-pointer entry point refuses such a
    value with its index, before anything is launched -- the output is untouched."""
    from uzkge_amd import UzkgeError
    from uzkge_amd import _native as N
    (w, perm, group, k, beta, gamma), _ = _z_inputs(2049, 5)
    for at, value in (((4, 2048), 5 * 2049), ((0, 0), 0xFFFFFFFF), ((2, 7), 8 * 2049)):
        bad = perm.copy()
        bad[at] = value
        with pytest.raises(UzkgeError) as e:
            gpu.z_poly(w, bad, group, k, beta, gamma)
        assert e.value.code == N.UZK_ERR_PARAMETER and f"perm[{at[0] * 2049 + at[1]}]" in str(e.value), str(e.value)
    ok = perm.copy()
    ok[4, 2048] = 5 * 2049 - 1                               # the largest value there is
    assert np.array_equal(gpu.z_poly(w, ok, group, k, beta, gamma), oc.z_poly(w, ok, group, k, beta, gamma))


# ---- zero factors in the grand product -------------------------------------------------------------------------------------------
# Inputs from tests/zero_factor.py (held to a Python-integer restatement by tests/test_zero_factor_helper.py, without a GPU).
@pytest.fixture(scope="module", params=[4097, 65538])
def zcase(request):
    """One-launch path / two-level path.  The oracle's z of the untouched inputs is computed once."""
    import zero_factor as zf
    c = zf.Case(request.param, 5, seed=request.param)
    c.z_good = oc.z_poly(*c.wires())
    return c


def _row(c, name):
    return c.n - 2 if name == "n-2" else c.n - 1 if name == "n-1" else int(name)


@pytest.mark.parametrize("row", ["0", "2047", "2048", "n-2"])
def test_z_poly_with_a_zero_numerator(gpu, zcase, row):
    """z is zero from row i + 1 on and the denominators are untouched: an ordinary call, equal to the oracle."""
    c, i = zcase, _row(zcase, row)
    w = c.with_zeros([("num", i, 2)])
    want = oc.z_poly(*c.wires(w))
    assert want[: i + 1].any(axis=1).all() and not want[i + 1:].any()          # the input does what it claims
    assert np.array_equal(gpu.z_poly(*c.wires(w)), want)


def test_z_poly_ignores_zero_factors_at_the_last_row(gpu, zcase):
    """Row n-1 takes no part in the product: a zero numerator AND a zero denominator there are accepted and change nothing."""
    c = zcase
    w = c.with_zeros([("num", c.n - 1, 0), ("den", c.n - 1, c.free_wire(c.n - 1, avoid=(0,)))])
    assert not np.array_equal(w, c.w_wire)
    got = gpu.z_poly(*c.wires(w))
    assert np.array_equal(got, oc.z_poly(*c.wires(w))) and np.array_equal(got, c.z_good)


@pytest.mark.parametrize("row", ["0", "2048", "n-2"])
def test_z_poly_refuses_a_zero_denominator_and_the_next_call_is_right(gpu, zcase, row):
    from uzkge_amd import UzkgeError
    from uzkge_amd import _native as N
    c, i = zcase, _row(zcase, row)
    w = c.with_zeros([("den", i, c.free_wire(i))])
    with pytest.raises(UzkgeError) as e:
        gpu.z_poly(*c.wires(w))
    assert e.value.code == N.UZK_ERR_PARAMETER and "denominator" in str(e.value), str(e.value)
    assert np.array_equal(gpu.z_poly(*c.wires()), c.z_good)                     # the same context, good inputs
