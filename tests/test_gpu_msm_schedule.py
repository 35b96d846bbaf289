"""The tapered end of the MSM's task schedule chooses a schedule, never a result.

uzk_tune("msm_taper"): the first buckets of every scan window are cut into short tasks (uzkge_amd/csrc/msm_cut.hpp): 0 never,
1 where the task list is several times the resident lanes (n = 2^24: a size no test should run), 2 at any size.  The tests
force it at the smallest sizes of the general pipeline: n = 2^16 + 3 (just above the small pipeline, a ragged last sort chunk)
and 2^18, at the automatic window width and at c = 11 and 17, the two-pass packed sort's narrowest and widest key.  A forced
run that trips a workspace guard raises: every test here is also a test of the host's bounds.

Every comparison is on canonical affine points (g1_to_affine) with np.array_equal, against the CPU oracle (one Pippenger per
(n, scalar set), shared by the tests) and against the same call with the switch at 0.  The degenerate bases are checked
against their closed form (tests/degenerate_msm.py).  The cutting rule itself, with the host's bounds, is tested on the CPU
(tests/test_msm_cut_host.py)."""
import contextlib

import numpy as np
import pytest
import torch

import bn254_py as opy
import degenerate_msm as dg
import oracle_c as oc
from util import affine_of

pytestmark = pytest.mark.gpu

N_SMALL, N_LARGE = (1 << 16) + 3, 1 << 18
SIZES = (N_SMALL, N_LARGE)
KINDS = ("uniform", "mix", "same", "zero", "one_nonzero")
WIDTHS = (0, 11, 17)
DEFAULTS = {"msm_taper": 1, "msm_stream_min_log": 22, "msm_stream_log": 0}


@contextlib.contextmanager
def tuned(gpu, window_bits=0, **keys):
    try:
        for k, v in keys.items():
            gpu.tune(k, v)
        gpu.set_msm_window_bits(window_bits)
        yield
    finally:
        for k in keys:
            gpu.tune(k, DEFAULTS[k])
        gpu.set_msm_window_bits(0)


class Data:
    """2^18 distinct random bases on the device (every size is a prefix), the scalar sets on the host, the oracle's answers"""

    def __init__(self, gpu):
        self.gpu = gpu
        n = N_LARGE
        self.pts = torch.empty((n, 8), dtype=torch.int64, device="cuda")
        sc = torch.empty((2, n, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        gpu.synth_points_random(self.pts.data_ptr(), n, 1601)
        gpu.synth_scalars(sc[0].data_ptr(), n, 1602)
        gpu.synth_scalars_mix(sc[1].data_ptr(), n, 1603)
        self.srs = gpu.Srs.from_device(self.pts.data_ptr(), n)
        self.wire = self.pts.cpu().numpy().view(np.uint64)
        host = sc.cpu().numpy().view(np.uint64)
        same = np.repeat(oc.fr_from_ints([0x1234567890ABCDEF1234567890ABCDEF0FEDCBA987654321 % opy.R]), n, axis=0)
        lone = np.zeros((n, 4), dtype=np.uint64)
        lone[40000] = host[0][5]
        self.sets = {"uniform": host[0], "mix": host[1], "same": same, "zero": np.zeros((n, 4), dtype=np.uint64), "one_nonzero": lone}
        self._want = {}

    def scalars(self, kind, n):
        return np.ascontiguousarray(self.sets[kind][:n])

    def want(self, kind, n):
        """canonical affine point of the CPU oracle's Pippenger, computed once"""
        if (kind, n) not in self._want:
            ref = self.gpu.g1_to_affine(oc.msm_pippenger(self.wire[:n], self.scalars(kind, n), 0, 8))
            ref.setflags(write=False)
            self._want[(kind, n)] = ref
        return self._want[(kind, n)]

    def run(self, kind, n):
        return self.gpu.g1_to_affine(self.gpu.msm(self.srs, self.scalars(kind, n)))


@pytest.fixture(scope="module")
def data(gpu):
    d = Data(gpu)
    yield d
    d.srs.release()


def scope_counts(gpu, run):
    gpu.profile_reset()
    gpu.profile_enable(True)
    try:
        out = run()
    finally:
        gpu.profile_enable(False)
    table = {k: v[0] for k, v in gpu.profile_table().items()}
    gpu.profile_reset()
    return out, table


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_taper_forced(gpu, data, n, kind):
    """uniform scalars, the prover-like mix, all scalars equal (one bucket per window holds every point: the big-bucket list,
    several fold levels and the cut rule meet), all zero, one nonzero scalar -- at every window width"""
    want = data.want(kind, n)
    for c in WIDTHS:
        with tuned(gpu, c, msm_taper=0):
            off = data.run(kind, n)
        with tuned(gpu, c, msm_taper=2):
            got = data.run(kind, n)
        assert np.array_equal(off, want), (c, "taper off")
        assert np.array_equal(got, want), (c, "taper forced")


@pytest.mark.parametrize("family,kind", [("one_point", "uniform"), ("plus_minus", "cancel"), ("pool64", "uniform"), ("one_point", "same")])
def test_taper_forced_on_degenerate_bases(gpu, family, kind):
    """repeated points and opposite pairs: short tasks reach the exception list and the folds' doubling / cancelling branches"""
    c = dg.case(family, kind, N_SMALL)
    srs = gpu.Srs.from_host(c.points)
    try:
        for width in (0, 17):
            with tuned(gpu, width, msm_taper=2):
                assert affine_of(gpu.msm(srs, c.scalars)) == c.want, width
    finally:
        srs.release()


def test_taper_forced_in_accumulating_chunks(gpu, data):
    """the streamed host-scalar call: four point chunks of 2^16 share one bucket set, every later one is added onto the first"""
    n = N_LARGE
    want = data.want("uniform", n)
    with tuned(gpu, 0, msm_taper=2, msm_stream_min_log=12, msm_stream_log=16):
        (got, table) = scope_counts(gpu, lambda: data.run("uniform", n))
        assert table.get("msm_accumulate", 0) == 4, table          # four chunks ran
        gpu.tune("msm_taper", 0)
        off = data.run("uniform", n)
    assert np.array_equal(got, want) and np.array_equal(off, want)


def test_taper_forced_in_a_batch(gpu, data):
    n = N_SMALL
    kinds = ("uniform", "mix", "same")
    vecs = np.stack([data.scalars(k, n) for k in kinds])
    with tuned(gpu, 0, msm_taper=2):
        out = gpu.msm_batch(data.srs, vecs)
    for k, o in zip(kinds, out):
        assert np.array_equal(gpu.g1_to_affine(o), data.want(k, n)), k


def test_switch_values(gpu):
    """0, 1 and 2 are the switch's values; unknown keys are still rejected (the window-group sort switch was measured and not kept)"""
    for v in (0, 2, 1):
        gpu.tune("msm_taper", v)
    for key in ("msm_taper_length", "msm_sort_group"):
        with pytest.raises(Exception):
            gpu.tune(key, 1)
