"""GPU: the Baby Jubjub layer -- uzk_ed_check_points, uzk_ed_mul_batch, uzk_ed_sum_batch, uzk_ed_unmask_batch -- bit for bit against
tests/ed_ref.py: the sizes at the kernels' edges (one lane per item, 64 lanes per workgroup), every edge scalar on every edge point,
every status at lanes 0, 63 and 64, sums that double and sums that cancel, and the reference's golden aggregate and unmask cases."""
import functools
import random

import numpy as np
import pytest

import ed_ref as e

pytestmark = pytest.mark.gpu
Q, L, G = e.Q, e.L, e.G
SIZES = (1, 63, 64, 65, 129)                                         # 129: one past the second workgroup


@functools.lru_cache(maxsize=None)
def _mul(k, p):
    return e.mul(k, p)


@functools.lru_cache(maxsize=None)
def _pool():
    """40 subgroup points -- made once, never changed"""
    return tuple(e.rand_subgroup_points(40, "gpu-edwards"))


@functools.lru_cache(maxsize=None)
def _edge_points():
    return (e.IDENTITY, e.ORDER2, e.ORDER4[0], e.ORDER4[1], e.order8_point(), G, e.neg(G), _pool()[0], _pool()[1], e.add(G, e.ORDER2))


def _edge_scalars():
    rng = random.Random("gpu-edwards-scalars")
    return [0, 1, 2, L - 1, L, L + 1, 1 << 251, (1 << 256) - 1, rng.randrange(1 << 256), rng.randrange(L)]


def test_every_edge_scalar_on_every_edge_point(gpu):
    items = [(k, p) for k in _edge_scalars() for p in _edge_points()]
    got = gpu.ed_mul_batch(e.points_wire([p for _, p in items]), e.scalars_wire([k for k, _ in items]))
    assert np.array_equal(got, e.points_wire([_mul(k, p) for k, p in items]))
    assert e.points_unwire(got[:len(_edge_points())]) == [e.IDENTITY] * len(_edge_points())       # 0 P, whatever P


@pytest.mark.parametrize("n", SIZES)
def test_mul_batch_sizes(gpu, n):
    pts, ks = _pool() + _edge_points(), _edge_scalars()
    rng = random.Random(f"gpu-edwards-mul-{n}")
    items = [(ks[(i + n) % len(ks)] if i % 3 else rng.randrange(1 << 256), pts[(5 * i + n) % len(pts)]) for i in range(n)]
    got = gpu.ed_mul_batch(e.points_wire([p for _, p in items]), e.scalars_wire([k for k, _ in items]))
    assert np.array_equal(got, e.points_wire([_mul(k, p) for k, p in items]))


@pytest.mark.parametrize("n", SIZES)
def test_mul_batch_with_one_shared_base(gpu, n):
    ks = _edge_scalars()
    rng = random.Random(f"gpu-edwards-shared-{n}")
    scalars = [ks[i % len(ks)] if i % 2 else rng.randrange(L) for i in range(n)]
    for base in (G, e.add(G, e.ORDER2)):
        got = gpu.ed_mul_batch(e.points_wire([base])[0], e.scalars_wire(scalars))
        assert np.array_equal(got, e.points_wire([_mul(k, base) for k in scalars]))


def _bad_rows():
    """wire rows of points with status 1, 2 and 3 (several of each)"""
    two = lambda x, y: np.concatenate([x, y])
    gx, gy = e.fr_wire([G[0]])[0], e.fr_wire([G[1]])[0]
    one = [two(e.raw_wire([Q])[0], gy), two(gx, e.raw_wire([Q + 5])[0]), two(e.raw_wire([(1 << 256) - 1])[0], e.raw_wire([(1 << 256) - 1])[0])]
    off = [e.points_wire([p])[0] for p in ((2, 3), (0, 0), (G[0], (G[1] + 1) % Q))]
    low = [e.points_wire([p])[0] for p in (e.ORDER2, e.ORDER4[1], e.order8_point(), e.add(G, e.ORDER2), e.add(_pool()[3], e.ORDER4[0]))]
    return {1: one, 2: off, 3: low}


@pytest.mark.parametrize("n", SIZES)
def test_check_points_accepts_subgroup_points(gpu, n):
    pts = [(_pool() + (e.IDENTITY, G))[i % 42] for i in range(n)]
    assert not gpu.ed_check_points(e.points_wire(pts)).any()


@pytest.mark.parametrize("turn", range(3))
def test_check_points_every_status_at_lanes_0_63_64(gpu, turn):
    bad = _bad_rows()
    wire = e.points_wire([_pool()[i % 40] for i in range(65)])
    want = [0] * 65
    for slot, lane in enumerate((0, 63, 64)):
        st = (turn + slot) % 3 + 1
        wire[lane] = bad[st][turn % len(bad[st])]
        want[lane] = st
    assert list(gpu.ed_check_points(wire)) == want


def test_check_points_every_bad_row(gpu):
    bad = _bad_rows()
    rows = [(st, r) for st in (1, 2, 3) for r in bad[st]]
    assert list(gpu.ed_check_points(np.stack([r for _, r in rows]))) == [st for st, _ in rows]


def _rows(k, n, seed):
    """k rows of n points: column j doubles (rows 0 and 1 equal) when j % 4 == 1, cancels (row 1 = -row 0) when j % 4 == 2, and
    cancels to the identity altogether when j % 4 == 3 and k == 4"""
    pool = _pool() + (e.IDENTITY, e.ORDER2, e.add(G, e.ORDER4[0]))
    rng = random.Random(f"gpu-edwards-rows-{k}-{n}-{seed}")
    rows = [[pool[rng.randrange(len(pool))] for _ in range(n)] for _ in range(k)]
    if k >= 2:
        for j in range(n):
            if j % 4 == 1:
                rows[1][j] = rows[0][j]
            elif j % 4 == 2:
                rows[1][j] = e.neg(rows[0][j])
            elif j % 4 == 3 and k == 4:
                rows[1][j], rows[3][j] = e.neg(rows[0][j]), e.neg(rows[2][j])
    return rows


def _rows_wire(rows):
    return np.stack([e.points_wire(r) for r in rows])


@pytest.mark.parametrize("k", (1, 4))
@pytest.mark.parametrize("n", SIZES)
def test_sum_and_unmask(gpu, k, n):
    rows = _rows(k, n, "sum")
    e2 = [_pool()[(3 * j + k) % 40] if j % 5 else rows[0][j] for j in range(n)]
    want_sum = [e.psum([rows[r][j] for r in range(k)]) for j in range(n)]
    assert np.array_equal(gpu.ed_sum_batch(_rows_wire(rows)), e.points_wire(want_sum))
    if k == 4 and n > 3:
        assert want_sum[3] == e.IDENTITY
    want = [e.unmask(e2[j], [rows[r][j] for r in range(k)]) for j in range(n)]
    assert np.array_equal(gpu.ed_unmask_batch(e.points_wire(e2), _rows_wire(rows)), e.points_wire(want))


def test_golden_aggregate_and_unmask(gpu):
    g = e.golden()
    got = gpu.ed_sum_batch(e.points_wire(g["keys"]).reshape(4, 1, 8))
    assert e.points_unwire(got) == [g["keys_sum"]]
    m = g["unmask_masked"]
    card = e.points_unwire(gpu.ed_unmask_batch(e.points_wire([(m[0], m[1])]), e.points_wire(g["unmask_reveals"]).reshape(4, 1, 8)))[0]
    assert card[1] == g["unmask_y"] and card == e.unmask((m[0], m[1]), g["unmask_reveals"])
    from uzkge_amd import reveal as rv
    assert rv.aggregate_keys(g["keys"]) == g["keys_sum"]
    assert rv.unmask([((m[2], m[3]), (m[0], m[1]))], [[p] for p in g["unmask_reveals"]]) == [card]
