"""The CPU oracle on degenerate base sets (tests/degenerate_msm.py): repeated bases, opposite pairs, infinities and powers of
two of one point, under every scalar kind.  oc.msm_pippenger -- the reference of the GPU MSM tests and the CPU baseline of the
benchmark -- and oc.msm_naive must agree with the closed form (sum s_i k_i mod r) * G, which is Python integers and one scalar
multiplication: this pins the checker itself on the inputs the GPU tests of test_gpu_msm_degenerate.py use."""
import pytest

import degenerate_msm as dg
from util import affine_of

import oracle_c as oc

N = 1 << 14

INFINITE = {("one_point", "cancel"), ("plus_minus", "same"), ("plus_minus", "cancel")}


@pytest.mark.parametrize("kind", dg.KINDS)
@pytest.mark.parametrize("family", dg.FAMILIES)
def test_oracle_matches_closed_form(family, kind):
    c = dg.case(family, kind, N)
    assert (c.want is None) == ((family, kind) in INFINITE)
    assert affine_of(oc.msm_pippenger(c.points, c.scalars, 0, 8)) == c.want
    assert affine_of(oc.msm_pippenger(c.points, c.scalars, 13, 1)) == c.want
    m = 512
    assert affine_of(oc.msm_naive(c.points[:m], c.scalars[:m])) == dg.closed_form(c.logs, c.idx[:m], c.ints[:m])


def test_block_signs_cancel_chunk_against_chunk():
    """plus_minus in block form with scalars of the same period: every block cancels the one before it"""
    p = 1 << 12
    even = dg.case("plus_minus", "periodic", 4 * p, base_period=p, scalar_period=p)
    assert even.want is None
    assert affine_of(oc.msm_pippenger(even.points, even.scalars, 0, 8)) is None
    odd = dg.case("plus_minus", "periodic", 3 * p + 5, base_period=p, scalar_period=p)
    assert odd.want is not None
    assert affine_of(oc.msm_pippenger(odd.points, odd.scalars, 0, 8)) == odd.want
    # three blocks (+, -, +) leave one block's sum, the ragged tail subtracts its own five terms
    one = dg.closed_form(odd.logs, odd.idx[:p], odd.ints[:p])
    assert affine_of(oc.msm_pippenger(odd.points[:3 * p], odd.scalars[:3 * p], 0, 8)) == one
