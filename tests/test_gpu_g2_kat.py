"""The device's Fq2 arithmetic and G2 group law (csrc/fq2_29.hpp, g2_29.hpp) through uzk_test_g2_kat, against the frozen results of
tests/golden/vectors_g2.npz (tests/g2_ref.py, Python integers).  Bit-exact: canonical words, no tolerance."""
import os

import numpy as np
import pytest

import g2_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vec(golden_dir):
    return np.load(os.path.join(golden_dir, "vectors_g2.npz"))


@pytest.mark.parametrize("op", sorted(gc.FQ2_OPS))
def test_fq2_ops_on_edge_and_random_operands(gpu, vec, op):
    """0, 1, u, p - 1, (p - 1) + (p - 1) u and limb-boundary values in every pairing, then random pairs; op 0 (two dual products)
    and op 5 (Karatsuba) are the two forms of the product and must give the same words"""
    got = gpu.g2_op(op, vec["fq2_a"], vec["fq2_b"])
    assert np.array_equal(got, vec[f"fq2_op{op}"])


@pytest.mark.parametrize("op", gc.GROUP_OPS)
def test_group_ops_cover_every_branch(gpu, vec, op):
    """P + Q, P + P (the doubling branch of the addition), P + (-P), infinity on either side and on both; a + b by the accumulator's
    mixed addition (10) and by the full XYZZ addition (11), 2a (12), a - b (13), 2(a + b) (14)"""
    jac = gpu.g2_op(op, vec["grp_a"], vec["grp_b"])
    got = np.stack([gpu.g2_to_affine(j) for j in jac])
    want = vec[f"grp_op{op}"]
    assert np.array_equal(got, want)
    assert (~want.any(axis=1)).sum() >= 6              # the cancellations and infinity + infinity are among the cases


def test_bad_op_is_refused(gpu):
    from uzkge_amd import UzkgeError
    z = np.zeros((1, 16), dtype=np.uint64)
    for op in (-1, 6, 9, 15):
        with pytest.raises(UzkgeError):
            gpu.g2_op(op, z, z)
