"""The Groth16 prover (uzk_g16_*) past the reveal key's shape.  Everywhere else in the suite the domain is at most 8192, so a group
is always 128 proofs, every G1 MSM but one takes the small pipeline and the G2 MSM sees one point chunk.  Here:

  (a) n = 2^15, batch 130      groups of 63 (63 + 63 + 4: two group boundaries and a short last group); the K MSM has more than 2^15
                               points and runs batched through the general pipeline; 189 transforms of 2^15 per group
  (b) n = 2^16, batch 33       groups of 31 (31 + 2)
  (c) n = 8, m = 2^15 + 3      the rows of A, B1, B have 2^15 + 5 points: the G2 MSM sums two point chunks (the second of five points) in
                               front of its Horner chain, and the A MSM reads z through the strided-plus-tail view in the general pipeline
  (d) an unsatisfying witness  at n = 2^15: h is still the definition's, h[n - 1] != 0
  the plan                     the group size and the admission of the three G1 MSMs over the accepted key shapes up to the bounds of
                               uzk_g16_key_create (uzk_test_g16_plan: nothing is launched), where running a proof is out of reach

Expected proofs are closed forms under a key of known logarithms (tests/g16_pool.py; tests/test_g16_pool_host.py holds that form to
the restatement's prover), h comes from g16_ref.witness_map (the oracle's transforms).  A case draws two witnesses and cycles them
through its batch, with blinds (r, s) of its own for every proof.  Every comparison is bit-exact on canonical words."""
import ctypes

import numpy as np
import pytest

import g16_cases as gc
import g16_pool as gp
import g16_ref as gr
import oracle_c as oc
from test_gpu_g16_finish import blob_of, check_blobs

pytestmark = pytest.mark.gpu

R = gr.R
GROUP_ELEMS = 1 << 21          # csrc/groth16.hip kGroupElems
L = 7


class Case:
    """a system, its pool key, two witnesses with their h, and the batch that cycles them"""

    def __init__(self, name, batch, n, l, nc, n_free, n_define, m=None):
        self.name, self.batch = name, batch
        self.sy = gc.system(name, n, l, nc, n_free, n_define, m=m)
        self.key = gp.PoolKey(name, self.sy.m, l, n)
        self.zs = [gc.witness(self.sy, k) for k in range(2)]
        assert self.zs[0] != self.zs[1] and all(gc.satisfied(self.sy, z) for z in self.zs)
        self.hs = [gr.witness_map(self.sy.matrices(), l, z) for z in self.zs]
        assert all(len(h) == n and h[-1] == 0 for h in self.hs)
        self.sums = [gr.closed_form_sums(self.key.logs, l, z, h) for z, h in zip(self.zs, self.hs)]
        self.blinds = [gc.blinds(name, b) for b in range(batch)]
        assert len(set(self.blinds)) == batch
        zw = [oc.fr_from_ints(z) for z in self.zs]
        self.z = np.stack([zw[b % 2] for b in range(batch)])
        self.r, self.s = oc.fr_from_ints([r for r, _ in self.blinds]), oc.fr_from_ints([s for _, s in self.blinds])
        self._want = None

    def want(self):
        """[batch, 32]: the closed form of every proof"""
        if self._want is None:
            self._want = np.stack([gr.proof_to_wire(gr.points_of(*gr.closed_form_blind(self.sums[b % 2], self.key.logs, r, s)))
                                   for b, (r, s) in enumerate(self.blinds)])
            assert all(w[:8].any() and w[8:24].any() and w[24:].any() for w in self._want)
        return self._want

    def device_key(self, gpu):
        return gpu.Groth16Key.from_arrays(**self.key.from_arrays_args(self.sy))


@pytest.fixture(scope="module")
def case15():
    return Case("pool-2^15", 130, 1 << 15, L, (1 << 15) - L, 256, 64)


@pytest.fixture(scope="module")
def case16():
    return Case("pool-2^16", 33, 1 << 16, L, (1 << 16) - L, 256, 64)


@pytest.fixture(scope="module")
def case_wide():
    """the sizes of d8_full with m = 2^15 + 3 variables; one define constraint, so that the generator's four long rows fit the rest"""
    n, l, nc, n_free, _ = gc.CASES["d8_full"]
    return Case("pool-m2^15+3", 3, n, l, nc, n_free, 1, m=(1 << 15) + 3)


def _plan(m, l, nc):
    """uzk_test_g16_plan -> (group, lens, admitted)"""
    from uzkge_amd import _native as N
    from uzkge_amd.errors import check
    group, lens, adm = ctypes.c_uint32(0), (ctypes.c_uint64 * 3)(), (ctypes.c_int * 3)()
    check(N.lib.uzk_test_g16_plan(m, l, nc, ctypes.byref(group), lens, adm))
    return group.value, list(lens), list(adm)


def _both_finishes(key, case):
    """every proof of the batch by both finishes against the closed form; every blob against its definition"""
    want = case.want()
    host = key.prove(case.z, case.r, case.s)
    dev, blobs = key.prove(case.z, case.r, case.s, finish="device")
    assert host.shape == dev.shape == (case.batch, 32)
    for b in range(case.batch):
        assert np.array_equal(host[b], want[b]), ("host finish", b)
        assert np.array_equal(dev[b], want[b]), ("device finish", b)
    assert np.array_equal(dev[:, 8:24], host[:, 8:24])              # the device finish's B is the affine of the host finish's
    check_blobs(dev, blobs)
    return dev, blobs


def test_domain_2_15_batch_130(gpu, case15):
    """(a): the row of K has 321 + 2^15 points, so a group is 2^21 // 33089 = 63 proofs and the batch runs as 63 + 63 + 4.  Both
    finishes; the device-assignment entry with the blobs left on the device, read back on both sides of every group boundary"""
    c = case15
    group = _plan(c.sy.m, L, c.sy.nc)[0]
    assert c.sy.m == 328 and group == GROUP_ELEMS // (321 + (1 << 15)) == 63 and 2 * group < c.batch
    with c.device_key(gpu) as key:
        assert key.domain == 1 << 15
        dev, blobs = _both_finishes(key, c)
        d_z, d_blobs = gpu.dev_alloc(c.z.nbytes), gpu.dev_alloc(c.batch * 256)
        try:
            gpu.dev_upload(d_z, c.z)
            pd, bd = key.prove_device(d_z, c.r, c.s, finish="device", d_blobs=d_blobs)
            assert np.array_equal(pd, dev) and np.array_equal(bd, blobs)
            left = gpu.dev_download(d_blobs, (c.batch, 256), dtype=np.uint8)
            for b in sorted({0, group - 1, group, 2 * group - 1, 2 * group, 63, 64, 127, 128, 129}):
                assert bytes(left[b]) == blob_of(c.want()[b]), b
        finally:
            gpu.dev_free(d_z)
            gpu.dev_free(d_blobs)


def test_witness_map_2_15_batch_130(gpu, case15):
    """(a): uzk_g16_h_device over the same batch, every row against the restatement (the rows of a group land at d_h + b0 n)"""
    c = case15
    hw = [oc.fr_from_ints(h) for h in c.hs]
    assert not np.array_equal(hw[0], hw[1])
    with c.device_key(gpu) as key:
        got = key.h(c.z)
    assert got.shape == (c.batch, 1 << 15, 4)
    for b in range(c.batch):
        assert np.array_equal(got[b], hw[b % 2]), b


def test_domain_2_16_batch_33(gpu, case16):
    """(b): a group is 2^21 // (321 + 2^16) = 31 proofs, the batch runs as 31 + 2; both finishes"""
    c = case16
    assert _plan(c.sy.m, L, c.sy.nc)[0] == GROUP_ELEMS // (321 + (1 << 16)) == 31 < c.batch
    with c.device_key(gpu) as key:
        assert key.domain == 1 << 16
        _both_finishes(key, c)


def test_two_g2_point_chunks(gpu, case_wide):
    """(c): rows of 2^15 + 5 points, batch 3, both finishes"""
    c = case_wide
    group, lens, adm = _plan(c.sy.m, c.sy.l, c.sy.nc)
    assert lens == [(1 << 15) + 5, (1 << 15) + 5, c.sy.m - c.sy.l + 8] and group == GROUP_ELEMS // max(lens) == 63 and adm == [1, 1, 1]
    with c.device_key(gpu) as key:
        assert (key.domain, key.n_vars) == (8, (1 << 15) + 3)
        _both_finishes(key, c)


def test_an_unsatisfying_witness_at_2_15(gpu, case15):
    """(d): one output variable bent.  h is the definition's and its top coefficient is not zero; a batch that mixes it with a
    satisfying assignment keeps both rows"""
    c = case15
    _, out, _ = c.sy.defines[len(c.sy.defines) // 2]
    bad = list(c.zs[0])
    bad[out] = (bad[out] + 1) % R
    assert not gc.satisfied(c.sy, bad)
    want = gr.witness_map(c.sy.matrices(), L, bad)
    assert want[-1] != 0
    with c.device_key(gpu) as key:
        got = key.h(np.stack([oc.fr_from_ints(bad), oc.fr_from_ints(c.zs[1])]))
    assert got[0, -1].any() and np.array_equal(got[0], oc.fr_from_ints(want))
    assert np.array_equal(got[1], oc.fr_from_ints(c.hs[1]))


# ---- the plan over the accepted shapes ---------------------------------------------------------------------------------------------
TOTALS = (8, 1 << 14, (1 << 14) + 1, 1 << 15, 1 << 16, 1 << 20, 1 << 21, (1 << 21) + 1, 1 << 25)         # n_constraints + l
VARS = (L, (1 << 15) - 2, (1 << 15) - 1, 1 << 19, (1 << 20) - 3, (1 << 20) - 2)                           # m


def test_the_group_plan_over_the_accepted_shapes(gpu):
    """Every shape uzk_g16_key_create accepts gets a group whose three G1 MSMs the MSM code admits (by its own admission function, at
    batch = group) and whose longest row stays within 2^21 elements per group, or is a group of one; the shapes measured so far keep
    their group of 128; what creation refused it still refuses."""
    from uzkge_amd import UzkgeError, _native as N
    cells = []
    for total in TOTALS:
        for m in VARS:
            nc = total - L
            n = gr.domain_of(nc, L)
            group, lens, adm = _plan(m, L, nc)
            assert lens == [m + 2, m + 2, (m - L) + n], (total, m)
            cells.append((total, m, group, adm, group * max(n, m + 2, (m - L) + n)))
    for total, m, group, adm, span in cells:
        print(f"n_constraints + l = {total}, m = {m}: group {group}, admitted {adm}, group * longest row = {span}")
    refused = [(total, m, group, adm) for total, m, group, adm, _ in cells if adm != [1, 1, 1] or group < 1]
    assert not refused, refused
    too_long = [(total, m, group, span) for total, m, group, _, span in cells if span > GROUP_ELEMS and group != 1]
    assert not too_long, too_long
    n, l, nc, m = gc.REAL
    assert _plan(m, l, nc)[0] == N.G16_GROUP == 128
    for name, (n, l, nc, n_free, n_define) in gc.CASES.items():
        assert _plan(l + n_free + n_define + 1, l, nc) == (128, [l + n_free + n_define + 3] * 2 + [n_free + n_define + 1 + n], [1, 1, 1]), name
    # refused as before: by the hook's shape rules, which are uzk_g16_key_create's, and by uzk_g16_key_create itself (the sizes are
    # judged before any array is looked at)
    tiny = np.zeros((1, 16), dtype=np.uint64)
    ptr = np.zeros(2, dtype=np.uint64)
    for m, nc in (((1 << 20) - 1, 1), (L, (1 << 25) + 1 - L)):
        with pytest.raises(UzkgeError) as e:
            _plan(m, L, nc)
        assert e.value.kind == "DegreeError"
        d, keep = gpu.Groth16Key.describe(m, L, nc, tiny[0, :8], tiny[0, :8], tiny[0, :8], tiny[0], tiny[0], tiny[:, :8], tiny[:, :8], tiny[:, :8], tiny[:, :8],
                                          tiny, [(ptr, np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=np.uint64))] * 3)
        h = ctypes.c_uint64(0)
        assert N.lib.uzk_g16_key_create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_DEGREE
        del keep
    with pytest.raises(UzkgeError) as e:
        _plan(L, L + 1, 1)
    assert e.value.kind == "ParameterError"
