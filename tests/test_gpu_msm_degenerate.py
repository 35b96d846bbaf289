"""The MSM on degenerate base sets, through every pipeline.

The other MSM tests feed bases that are pairwise distinct and never opposite, so the code that handles a degenerate group
addition -- the accumulator's exception list and its redo pass, the doubling / cancellation branches inside the fold levels and
the bucket reductions, `prev + acc` of the accumulating chunks, equal entries of a window table -- almost never runs there.
Here the bases repeat, come in opposite pairs, hold infinities, or are powers of two of one point (tests/degenerate_msm.py), and
every assertion is  affine(GPU result) == (sum s_i k_i mod r) * G  -- Python integers over the known discrete logs, no second
Pippenger (tests/test_oracle_degenerate.py holds the CPU oracle to the same closed form).

Sizes are the smallest that reach the path named in each section; nothing exceeds 2^18 points.  Every section but the sharded
one (its shards have contexts of their own) runs under uzk_tune("arith29") 7 and 0: the folds and reductions exist in both
arithmetics."""
import contextlib

import numpy as np
import pytest

import bn254_py as opy
import degenerate_msm as dg
from util import affine_of

pytestmark = pytest.mark.gpu

MASKS = (7, 0)
DEFAULTS = {"arith29": 7, "msm_small": 1, "msm_no_precompute": 0, "msm_stream_min_log": 22, "msm_stream_log": 0, "msm_chunk_log": 26}


@contextlib.contextmanager
def tuned(gpu, window_bits=None, **keys):
    """uzk_tune switches (and the forced window width) for the block, the defaults back afterwards whatever happens"""
    try:
        for k, v in keys.items():
            gpu.tune(k, v)
        if window_bits is not None:
            gpu.set_msm_window_bits(window_bits)
        yield
    finally:
        for k in keys:
            gpu.tune(k, DEFAULTS[k])
        if window_bits is not None:
            gpu.set_msm_window_bits(0)


@contextlib.contextmanager
def registered(gpu, points):
    srs = gpu.Srs.from_host(points)
    try:
        yield srs
    finally:
        srs.release()


def check_masks(gpu, run, want, tag):
    """run() under both arithmetics: each result is the closed form"""
    for mask in MASKS:
        with tuned(gpu, arith29=mask):
            got = affine_of(run())
        assert got == want, (tag, "arith29", mask)


def scopes(gpu, run):
    """(run(), how often every profiled scope ran inside it)"""
    gpu.profile_reset()
    gpu.profile_enable(True)
    try:
        out = run()
    finally:
        gpu.profile_enable(False)
    table = {k: v[0] for k, v in gpu.profile_table().items()}
    gpu.profile_reset()
    return out, table


COMBOS = [(f, k) for f in dg.FAMILIES for k in dg.KINDS]
combos = pytest.mark.parametrize("family,kind", COMBOS, ids=[f"{f}-{k}" for f, k in COMBOS])


# ---- a. the small pipeline (n <= 2^15): one workgroup per (vector, window) slot --------------------------------------------
@combos
def test_small_pipeline(gpu, family, kind):
    """n = 4096, general mode and over the window table of uzk_srs_precompute(0)"""
    c = dg.case(family, kind, 4096)
    with registered(gpu, c.points) as srs:
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "plain")
        srs.precompute(0)
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "table")


@pytest.mark.parametrize("n", [2, 3, 64])
@pytest.mark.parametrize("family", ["one_point", "plus_minus"])
def test_small_pipeline_raw_bases(gpu, family, n):
    """uzk_msm_g1_raw takes any bases: two, three and 64 copies of +-P under every scalar kind"""
    for kind in dg.KINDS:
        c = dg.case(family, kind, n)
        check_masks(gpu, lambda: gpu.msm_raw(c.points, c.scalars), c.want, (kind, "raw"))
        with registered(gpu, c.points) as srs:
            srs.precompute(0)
            check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, (kind, "table"))


@pytest.mark.parametrize("family,kind", [("one_point", "uniform"), ("plus_minus", "cancel")])
def test_small_pipeline_at_its_largest_size(gpu, family, kind):
    c = dg.case(family, kind, 1 << 15)
    with registered(gpu, c.points) as srs:
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "plain")
        srs.precompute(0)
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "table")


def test_small_pipeline_batch(gpu):
    """one uzk_msm_g1_batch call: three vectors over the same repeated base, one of them summing to infinity"""
    cases = [dg.case("one_point", kind, 4096) for kind in ("uniform", "same", "cancel")]
    assert cases[2].want is None
    vecs = np.stack([c.scalars for c in cases])
    with registered(gpu, cases[0].points) as srs:
        for table in (False, True):
            if table:
                srs.precompute(0)
            for mask in MASKS:
                with tuned(gpu, arith29=mask):
                    out = gpu.msm_batch(srs, vecs)
                assert [affine_of(o) for o in out] == [c.want for c in cases], (table, mask)


# ---- b. the general pipeline at c = 8 ---------------------------------------------------------------------------------------
@combos
def test_general_pipeline_forced_at_4096(gpu, family, kind):
    c = dg.case(family, kind, 1 << 12)
    with registered(gpu, c.points) as srs, tuned(gpu, msm_small=0):
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "general")


@pytest.mark.parametrize("family,kind,period", [
    ("one_point", "uniform", None),     # every task of two or more points is an exception: the list fills close to its bound
    ("one_point", "periodic", 4096),
    ("one_point", "same", None),        # ONE bucket per window holds all n points: two extra fold levels, every partial sum equal
    ("plus_minus", "cancel", None),
    ("pool64", "uniform", None),        # sparse degeneracy: exceptions next to tasks that stay on the fast path
])
def test_general_pipeline_at_its_natural_size(gpu, family, kind, period):
    n = (1 << 16) + 1
    assert gpu.msm_plan_info(n) == (8, 32)
    c = dg.case(family, kind, n, scalar_period=period)
    with registered(gpu, c.points) as srs:
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "general")


# ---- c. the class-sum reduction and directly written buckets (c >= 13) ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "pow2", "cancel"])
@pytest.mark.parametrize("family", dg.FAMILIES)
def test_class_sum_reduction(gpu, family, kind):
    """n = 2^17 at the default c = 15: eight points per bucket on average and tasks of >= 16, so nearly every bucket is one task
    that the accumulator -- or, for an exception, its redo pass -- writes straight into the bucket array"""
    n = 1 << 17
    assert gpu.msm_plan_info(n) == (15, 17)
    c = dg.case(family, kind, n)
    with registered(gpu, c.points) as srs:
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "c15")


@pytest.mark.parametrize("bits", [13, 16])
def test_class_sum_reduction_other_widths(gpu, bits):
    c = dg.case("one_point", "uniform", 1 << 17)
    with registered(gpu, c.points) as srs, tuned(gpu, window_bits=bits):
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, bits)


# ---- d. the window table in the general pipeline: T[j][i] = 2^(c j) P_i, one shared bucket set -------------------------------------
@pytest.mark.parametrize("family,kind", [("pow2", "pow2"), ("pow2", "uniform"), ("one_point", "uniform"), ("pool64", "uniform")])
@pytest.mark.parametrize("bits", [0, 20])
def test_window_table(gpu, bits, family, kind):
    """powers of two of one point put EQUAL entries at different (i, j) of the table, and they meet in the shared buckets"""
    c = dg.case(family, kind, 1 << 16)
    with registered(gpu, c.points) as srs:
        srs.precompute(bits)
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "table")
        with tuned(gpu, msm_no_precompute=1):
            assert affine_of(gpu.msm(srs, c.scalars)) == c.want


@pytest.mark.parametrize("family,kind", [("one_point", "uniform"), ("one_point", "same"), ("pow2", "pow2")])
def test_window_table_widest(gpu, family, kind):
    """c = 22: one set of 2^21 buckets, beyond the class sums and the scans -- the double-and-add reduction (msm_reduce_kernel)"""
    c = dg.case(family, kind, 4096)
    with registered(gpu, c.points) as srs:
        srs.precompute(22)
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "c22")


# ---- e. accumulating chunks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,kind,base_period,scalar_period,full", [
    ("one_point", "periodic", None, 1 << 16, 3),      # every chunk's bucket sums EQUAL what is already there: prev + acc doubles
    ("plus_minus", "periodic", 1 << 16, 1 << 16, 3),  # every chunk cancels the one before: prev + acc is infinity in every bucket
    ("pool64", "uniform", None, None, 3),
    ("one_point", "same", None, None, 3),             # one bucket per window: every chunk runs the extra fold levels before it adds
    # 512 values: 128 points per bucket and chunk (256 where two values share a digit), 8 .. 16 partial sums -- more than one lane
    # folds in the last level, too few for an extra level: one wave folds them (msm_fold_big_kernel) and ADDS its sum onto the
    # bucket, which holds the same sum, or its opposite
    ("one_point", "periodic", None, 512, 3),
    ("plus_minus", "periodic", 1 << 16, 512, 3),
    # +S, -S, +S ends as S whether a chunk adds or overwrites; with two full chunks the ragged one adds onto infinity everywhere
    ("plus_minus", "periodic", 1 << 16, 1 << 16, 2),
    ("plus_minus", "periodic", 1 << 16, 512, 2),
])
def test_streamed_chunks(gpu, family, kind, base_period, scalar_period, full):
    """host scalars streamed in point chunks (`full` x 2^16 and a ragged 5) into ONE bucket set"""
    n = full * (1 << 16) + 5
    c = dg.case(family, kind, n, base_period=base_period, scalar_period=scalar_period)
    with registered(gpu, c.points) as srs:
        with tuned(gpu, msm_stream_min_log=12, msm_stream_log=16):
            check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "streamed")
        with tuned(gpu, msm_stream_min_log=12, msm_stream_log=-1):
            assert affine_of(gpu.msm(srs, c.scalars)) == c.want


@pytest.mark.parametrize("family", ["one_point", "plus_minus"])
def test_dispatcher_chunk_loop(gpu, family):
    """uzk_tune("msm_chunk_log", 10): five MSMs of <= 1024 points whose results the host adds -- four equal ones (doubling), or
    four that cancel in pairs -- and a ragged fifth"""
    c = dg.case(family, "periodic", 4096 + 7, base_period=1024, scalar_period=1024)
    with registered(gpu, c.points) as srs, tuned(gpu, msm_chunk_log=10):
        check_masks(gpu, lambda: gpu.msm(srs, c.scalars), c.want, "chunk loop")


def test_sharded_equal_partials(gpu):
    """three shards of one device, the same points and scalars in each: three equal partial sums, folded to their triple"""
    p = 1 << 12
    c = dg.case("one_point", "periodic", 3 * p, scalar_period=p)
    sh = gpu.ShardedSrs(c.points, [0, 0, 0], -1)
    try:
        out, parts = sh.msm(c.scalars, want_partials=True)
    finally:
        sh.release()
    one = dg.closed_form(c.logs, c.idx[:p], c.ints[:p])
    assert one is not None
    assert [affine_of(q) for q in parts] == [one] * 3
    assert affine_of(out) == opy.g1_mul(one, 3) == c.want


# ---- the paths the sections above name are the ones that run ------------------------------------------------------------------------
def test_the_named_paths_run(gpu):
    """Profiled scope counts (uzk_profile_*): a case that silently moved to another pipeline would keep passing and test nothing."""
    c = dg.case("one_point", "same", 4096)
    with registered(gpu, c.points) as srs:
        _, t = scopes(gpu, lambda: gpu.msm(srs, c.scalars))
        assert t.get("msm_small_sort", 0) == 1 and "msm_finalize" not in t
        with tuned(gpu, msm_small=0):
            _, t = scopes(gpu, lambda: gpu.msm(srs, c.scalars))
        assert t.get("msm_finalize", 0) == 1 and "msm_small_sort" not in t
    # all 2^16 + 1 points in one bucket per window, tasks of 16: 4097 partial sums -> 129 -> 5: the copy of the directly written
    # sums back among the partial sums (msm_undirect_kernel) and two extra levels share the scope msm_combine
    c = dg.case("one_point", "same", (1 << 16) + 1)
    with registered(gpu, c.points) as srs:
        out, t = scopes(gpu, lambda: gpu.msm(srs, c.scalars))
        assert affine_of(out) == c.want
        assert t.get("msm_combine", 0) == 3 and "msm_reduce_class" not in t
    c = dg.case("one_point", "uniform", 1 << 17)
    with registered(gpu, c.points) as srs:
        _, t = scopes(gpu, lambda: gpu.msm(srs, c.scalars))
        assert t.get("msm_reduce_class", 0) == 1 and "msm_combine" not in t
    c = dg.case("one_point", "periodic", 3 * (1 << 16) + 5, scalar_period=1 << 16)
    with registered(gpu, c.points) as srs, tuned(gpu, msm_stream_min_log=12, msm_stream_log=16):
        _, t = scopes(gpu, lambda: gpu.msm(srs, c.scalars))
        assert t.get("host_msm_upload", 0) == 4 and t.get("msm_finalize", 0) == 4 and t.get("msm_reduce_class", 0) == 1
    c = dg.case("one_point", "periodic", 4096 + 7, base_period=1024, scalar_period=1024)
    with registered(gpu, c.points) as srs, tuned(gpu, msm_chunk_log=10):
        _, t = scopes(gpu, lambda: gpu.msm(srs, c.scalars))
        assert t.get("msm_small_sort", 0) == 5
