"""tests/zero_factor.py does what it claims: the wire value it sets makes exactly the chosen factor of the grand product zero, and
the oracle's z_poly (the reference of tests/test_gpu_poly_helpers.py) answers such an input the way a plain Python-integer
restatement of helpers.rs:160-220 does.  No GPU: this is the proof that the zero-factor inputs of the GPU tests are what they say."""
import copy

import numpy as np
import pytest

import oracle_c as oc
import zero_factor as zf


@pytest.fixture(scope="module", params=[16, 4097])
def case(request):
    return zf.Case(request.param, 5, seed=request.param)


def _oracle(case, w_ints):
    w_wire = oc.fr_from_ints([v for row in w_ints for v in row]).reshape(case.n_wires, case.n, 4)
    return oc.fr_to_ints(oc.z_poly(*case.wires(w_wire)))


def test_untouched_inputs_have_no_zero_factor_and_the_oracle_is_the_restatement(case):
    z, nums, dens = zf.restatement(*case.ints())
    assert all(nums) and all(dens) and all(z)
    assert _oracle(case, case.w) == z


@pytest.mark.parametrize("row", ["first", "middle", "last_used"])
def test_a_zero_numerator_gives_zero_from_the_next_row_on(case, row):
    n = case.n
    i = {"first": 0, "middle": n // 2, "last_used": n - 2}[row]
    for j in (0, case.n_wires - 1):
        w = copy.deepcopy(case.w)
        v = zf.zero_numerator(w, *case.ints()[1:], i, j)
        assert [(a, b) for a in range(case.n_wires) for b in range(n) if w[a][b] != case.w[a][b]] == [(j, i)] and w[j][i] == v
        z, nums, dens = zf.restatement(w, *case.ints()[1:])
        assert [t for t, x in enumerate(nums) if x == 0] == [i] and all(dens)
        assert all(z[: i + 1]) and not any(z[i + 1:]) and len(z) == n
        assert _oracle(case, w) == z


@pytest.mark.parametrize("row", ["first", "middle", "last_used"])
def test_a_zero_denominator_gives_a_zero_denominator_product(case, row):
    n = case.n
    i = {"first": 0, "middle": n // 2, "last_used": n - 2}[row]
    j = case.free_wire(i)
    w = copy.deepcopy(case.w)
    zf.zero_denominator(w, *case.ints()[1:], i, j)
    z, nums, dens = zf.restatement(w, *case.ints()[1:])
    assert z is None and [t for t, x in enumerate(dens) if x == 0] == [i] and all(nums)      # the numerator survives
    prod = 1
    for d in dens:
        prod = prod * d % zf.R
    assert prod == 0


def test_zeros_at_the_last_row_change_nothing(case):
    n = case.n
    j_den = case.free_wire(n - 1, avoid=(0,))
    w = copy.deepcopy(case.w)
    zf.zero_numerator(w, *case.ints()[1:], n - 1, 0)
    zf.zero_denominator(w, *case.ints()[1:], n - 1, j_den)
    assert w[0][n - 1] != case.w[0][n - 1] and w[j_den][n - 1] != case.w[j_den][n - 1]
    z, _, _ = zf.restatement(w, *case.ints()[1:])
    assert z == zf.restatement(*case.ints())[0] and _oracle(case, w) == z


def test_with_zeros_builds_the_same_witness_in_wire_format(case):
    n = case.n
    before = copy.deepcopy(case.w)
    j = case.free_wire(3)
    got = case.with_zeros([("num", 1, 2), ("den", 3, j)])
    assert case.w == before
    w = copy.deepcopy(case.w)
    zf.zero_numerator(w, *case.ints()[1:], 1, 2)
    zf.zero_denominator(w, *case.ints()[1:], 3, j)
    assert np.array_equal(got, oc.fr_from_ints([v for row in w for v in row]).reshape(case.n_wires, n, 4))


def test_the_gamma_that_zeroes_a_denominator():
    """zero_denominator_gamma over a real domain (group[i] = omega^i): exactly the chosen row's denominator vanishes."""
    import bn254_py as opy
    n = 16
    c = zf.Case(n, 5, seed=3)
    omega = opy.root_of_unity(n)
    group = [pow(omega, i, zf.R) for i in range(n)]
    i = 5
    j = c.free_wire(i)
    gamma = zf.zero_denominator_gamma(c.w[j][i], c.beta, c.k, omega, int(c.perm[j][i]), n)
    z, nums, dens = zf.restatement(c.w, c.perm, group, c.k, c.beta, gamma)
    assert z is None and [t for t, x in enumerate(dens) if x == 0] == [i] and all(nums)
