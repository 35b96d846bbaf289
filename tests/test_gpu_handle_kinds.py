"""GPU: the five kinds of process-wide key handle keep apart, on live handles.  One key of each kind, the smallest the API accepts --
a G2 base set of one point, a remask key, a Groth16 verifying key with one input, a PlonK verifier key with no public input over
a domain of two, the Groth16 proving key of the smallest case of tests/g16_cases.py -- is offered to the release and info entry points
of every other kind: each such call is UZK_ERR_PARAMETER and leaves the handle alive; its own release then works once."""
import ctypes
import os

import numpy as np
import pytest

import ed_ref as e
import g16_cases as gc

pytestmark = pytest.mark.gpu


def _g16_key(gpu, vec, name):
    _, l, nc, _, _ = gc.CASES[name]
    m = vec[f"{name}_a_query"].shape[0]
    return gpu.Groth16Key.from_arrays(
        m, l, nc, vec[f"{name}_alpha_g1"], vec[f"{name}_beta_g1"], vec[f"{name}_delta_g1"], vec[f"{name}_beta_g2"], vec[f"{name}_delta_g2"],
        vec[f"{name}_a_query"], vec[f"{name}_b_g1_query"], vec[f"{name}_l_query"], vec[f"{name}_h_query"], vec[f"{name}_b_g2_query"],
        [(vec[f"{name}_{t}_ptr"], vec[f"{name}_{t}_col"], vec[f"{name}_{t}_val"]) for t in "ABC"])


def test_no_kind_takes_another_kinds_live_handle(gpu, golden_dir):
    from uzkge_amd import _native as N
    lib = N.lib
    g1 = lambda count: np.zeros((count, 8), dtype=np.uint64)          # points at infinity: a key's points are taken as given
    fr = np.zeros(4, dtype=np.uint64)
    smallest = min(gc.CASES, key=lambda name: (gc.CASES[name][0], gc.CASES[name][2]))
    keys = {
        "g2": gpu.G2Bases.from_host(np.zeros((1, 16), dtype=np.uint64)),
        "remark": gpu.RemarkKey(e.points_wire([e.G])[0]),
        "g16_vk": gpu.Groth16VerifierKey(g1(1), np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64), np.zeros(16, dtype=np.uint64), g1(1)),
        "vk": gpu.VerifierKey(2, g1(9), g1(5), g1(1), g1(4), g1(1), np.zeros((5, 4), dtype=np.uint64), fr, fr, fr, fr, np.zeros((0, 4), dtype=np.uint64),
                              np.zeros((0, 4), dtype=np.uint64), shuffle=False),
        "g16_key": _g16_key(gpu, np.load(os.path.join(golden_dir, "vectors_g16.npz")), smallest),
    }
    size = ctypes.c_size_t(0)
    info = {
        "g2": lambda h: lib.uzk_g2_len(h, ctypes.byref(size)),
        "remark": lambda h: lib.uzk_remark_key_tables(h, None, None),
        "g16_vk": lambda h: lib.uzk_g16_vk_info(h, None, None),
        "vk": lambda h: lib.uzk_vk_info(h, None, None, None, None),
        "g16_key": lambda h: lib.uzk_g16_key_info(h, None, None, None, None, None),
    }
    release = {"g2": lib.uzk_g2_release, "remark": lib.uzk_remark_key_release, "g16_vk": lib.uzk_g16_vk_release, "vk": lib.uzk_vk_release,
               "g16_key": lib.uzk_g16_key_release}
    handles = {kind: key.handle for kind, key in keys.items()}
    try:
        assert len(set(handles.values())) == len(handles)
        assert keys["g2"].len() == 1 and keys["g16_vk"].info()[0] == 1 and keys["vk"].info()[:2] == (2, 0)
        assert (keys["g16_key"].domain, keys["g16_key"].n_constraints) == (gc.CASES[smallest][0], gc.CASES[smallest][2])
        for kind, h in handles.items():
            for other in handles:
                if other == kind:
                    continue
                assert info[other](h) == N.UZK_ERR_PARAMETER, (kind, other)
                assert release[other](h) == N.UZK_ERR_PARAMETER, (kind, other)
                assert info[kind](h) == N.UZK_OK, (kind, other)         # still alive
        for kind, h in handles.items():
            assert release[kind](h) == N.UZK_OK, kind
            keys[kind].handle = 0
            assert release[kind](h) == N.UZK_ERR_PARAMETER, kind
            assert info[kind](h) == N.UZK_ERR_PARAMETER, kind
            for other, ho in handles.items():                          # the others are as they were
                if keys[other].handle:
                    assert info[other](ho) == N.UZK_OK, (kind, other)
    finally:
        for key in keys.values():
            key.release()
