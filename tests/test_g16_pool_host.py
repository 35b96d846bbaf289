"""CPU check of the pool key (tests/g16_pool.py): the closed form it gives a proof (g16_ref.closed_form_logs over the key's known
logarithms) against the restatement's own prover -- the oracle's Pippenger MSMs and g2_ref.msm over the key's POINTS, decoded from the
very wire arrays a device key is made of.  That ties the reference of tests/test_gpu_g16_large.py to the one the suite already trusts."""
import numpy as np
import pytest

import g16_cases as gc
import g16_pool as gp
import g16_ref as gr

R = gr.R


def test_the_pool_holds_its_named_scalars():
    for group, size in (("g1", gp.POOL_G1), ("g2", gp.POOL_G2)):
        sc, wire = gp.table(group)
        assert len(sc) == size == wire.shape[0] and len(set(sc)) == size
        k = sc[3]
        assert sc[:3] == [0, 1, R - 1] and sc[4] == R - k and sc[5] == 2 * k % R and 1 < k < R - 1
        assert not wire[0].any() and all(wire[i].any() for i in range(1, size))            # only the scalar 0 is the infinity
    assert gp.pool("g1")[3] != gp.pool("g2")[3]


@pytest.mark.parametrize("name", ("d8_full", "d64_full"))
def test_the_restatements_prover_over_a_pool_key_equals_the_closed_form(name):
    sy = gc.case_system(name)
    key = gp.PoolKey(name, sy.m, sy.l, sy.n)
    for column in gp.COLUMNS:
        infinities, pairs, repeats = key.drawn(column)
        assert infinities >= 1 and pairs >= 1 and repeats >= 1, column                      # actually drawn, in every column
    assert key.logs["b1"] != key.logs["b2"] and key.logs["beta_g1"] != key.logs["beta_g2"] and key.logs["delta_g1"] != key.logs["delta_g2"]
    assert {len(key.logs[c]) for c in ("a", "b1", "b2")} == {sy.m} and len(key.logs["l"]) == sy.m - sy.l and len(key.logs["h"]) == sy.n - 1
    ref = key.ref_key()
    assert np.array_equal(gr.g1_to_wire(ref.h_query), key.arrays["h_query"]) and sum(p is None for p in ref.b_g2_query) >= 1
    for k in range(2):
        z = gc.witness(sy, k)
        r, s = gc.blinds(name, k)
        h = gr.witness_map(sy.matrices(), sy.l, z)
        got = gr.prove(ref, sy.matrices(), sy.l, z, r, s, h)
        want = gr.points_of(*gr.closed_form_logs(key.logs, sy.l, z, r, s, h))
        assert None not in got and got == want, k


def test_a_trapdoor_key_is_one_producer_of_the_logarithms():
    """closed_form is closed_form_logs over trapdoor_scalars; the blinds enter through closed_form_blind alone"""
    name = "d8_half"
    sy, trap = gc.case_system(name), gc.trapdoor(name)
    z = gc.witness(sy, 0)
    h = gr.witness_map(sy.matrices(), sy.l, z)
    logs = gr.trapdoor_scalars(sy.matrices(), sy.l, sy.m, trap)
    sums = gr.closed_form_sums(logs, sy.l, z, h)
    for k in range(2):
        r, s = gc.blinds(name, k)
        assert gr.closed_form(sy.matrices(), sy.l, z, r, s, trap, h) == gr.closed_form_logs(logs, sy.l, z, r, s, h) == gr.closed_form_blind(sums, logs, r, s)
