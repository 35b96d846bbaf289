"""The Groth16 prover (uzk_g16_*) against the frozen restatement of tests/golden/vectors_g16.npz (tests/g16_ref.py: Python integers and
the C oracle): the witness map at domain sizes 8, 64 and 1024 with the domain full and mostly zero rows, trapdoor proofs, the
reference's reveal key at its real shape, and the life of a key handle.  Every comparison is bit-exact on canonical words."""
import ctypes
import os

import numpy as np
import pytest

import g16_cases as gc
import g16_ref as gr
import oracle_c as oc

pytestmark = pytest.mark.gpu

NAMES = tuple(gc.CASES)


@pytest.fixture(scope="module")
def vec(golden_dir):
    return np.load(os.path.join(golden_dir, "vectors_g16.npz"))


def _key(gpu, vec, name):
    n, l, nc, _, _ = gc.CASES[name]
    m = vec[f"{name}_a_query"].shape[0]
    return gpu.Groth16Key.from_arrays(
        m, l, nc, vec[f"{name}_alpha_g1"], vec[f"{name}_beta_g1"], vec[f"{name}_delta_g1"], vec[f"{name}_beta_g2"], vec[f"{name}_delta_g2"],
        vec[f"{name}_a_query"], vec[f"{name}_b_g1_query"], vec[f"{name}_l_query"], vec[f"{name}_h_query"], vec[f"{name}_b_g2_query"],
        [(vec[f"{name}_{t}_ptr"], vec[f"{name}_{t}_col"], vec[f"{name}_{t}_val"]) for t in "ABC"])


@pytest.mark.parametrize("name", NAMES)
def test_witness_map(gpu, vec, name):
    """h of one assignment against the frozen h; batch 3 against three single calls; an unsatisfying assignment against the restatement
    (h[n - 1] != 0 there)"""
    with _key(gpu, vec, name) as key:
        assert (key.domain, key.n_inputs, key.n_constraints) == gc.CASES[name][:3]
        z = vec[f"{name}_z"]
        singles = [key.h(z[b:b + 1])[0] for b in range(gc.BATCH)]
        assert np.array_equal(singles[0], vec[f"{name}_h"])
        assert all(not h[-1].any() for h in singles)
        batch = key.h(z)
        for b in range(gc.BATCH):
            assert np.array_equal(batch[b], singles[b]), b
        bad = key.h(vec[f"{name}_z_bad"][None])[0]
        assert bad[-1].any() and np.array_equal(bad, vec[f"{name}_h_bad"])
        mixed = key.h(np.stack([z[1], vec[f"{name}_z_bad"], z[2]]))
        assert np.array_equal(mixed[1], vec[f"{name}_h_bad"]) and np.array_equal(mixed[2], singles[2])


@pytest.mark.parametrize("name", NAMES)
def test_trapdoor_proofs(gpu, vec, name):
    """batch 1 and 3 against the frozen proofs; r = s = 0 and r = s = r_mod - 1; the device-assignment entry against the host entry"""
    with _key(gpu, vec, name) as key:
        z, r, s = vec[f"{name}_z"], vec[f"{name}_r"], vec[f"{name}_s"]
        want = vec[f"{name}_proofs"]
        assert np.array_equal(key.prove(z[:1], r[:1], s[:1])[0], want[0])
        got = key.prove(z, r, s)
        for b in range(gc.BATCH):
            assert np.array_equal(got[b], want[b]), b
        zero, rm1 = oc.fr_from_ints([0]), oc.fr_from_ints([gr.R - 1])
        assert np.array_equal(key.prove(z[:1], zero, zero)[0], vec[f"{name}_proof_zero"])
        assert np.array_equal(key.prove(z[:1], rm1, rm1)[0], vec[f"{name}_proof_rm1"])
        d = gpu.dev_alloc(z.nbytes)
        try:
            gpu.dev_upload(d, z)
            assert np.array_equal(key.prove_device(d, r, s), want)
        finally:
            gpu.dev_free(d)


def test_a_second_context(gpu, vec):
    """a key made under a second context proves there; the context's workspaces die with it"""
    name = "d64_half"
    ctx = gpu.ctx_create_on(0)
    try:
        gpu.ctx_set_current(ctx)
        with _key(gpu, vec, name) as key:
            assert np.array_equal(key.prove(vec[f"{name}_z"], vec[f"{name}_r"], vec[f"{name}_s"]), vec[f"{name}_proofs"])
    finally:
        gpu.ctx_set_current(0)
        gpu.ctx_destroy(ctx)


def test_batch_across_the_group_boundary(gpu, vec):
    """batch 129 at domain 8: the second group holds one proof.  Proofs 0, 127 and 128 equal the closed form of the trapdoor key
    (tests/test_g16_ref_host.py holds the restatement's prover to that form), all 129 equal their single calls' frozen values where
    frozen"""
    name = "d8_full"
    sy, trap = gc.case_system(name), gc.trapdoor(name)
    zs = [gc.witness(sy, k) for k in range(gc.BIG_BATCH)]
    rs = [gc.blinds(name, k) for k in range(gc.BIG_BATCH)]
    with _key(gpu, vec, name) as key:
        got = key.prove(np.stack([oc.fr_from_ints(z) for z in zs]), oc.fr_from_ints([r for r, _ in rs]), oc.fr_from_ints([s for _, s in rs]))
    assert got.shape == (gc.BIG_BATCH, 32)
    for b in range(gc.BATCH):
        assert np.array_equal(got[b], vec[f"{name}_proofs"][b]), b
    for b in (0, 127, 128):
        h = gr.witness_map(sy.matrices(), sy.l, zs[b])
        want = gr.proof_to_wire(gr.points_of(*gr.closed_form(sy.matrices(), sy.l, zs[b], rs[b][0], rs[b][1], trap, h)))
        assert want.any() and np.array_equal(got[b], want), b


def test_the_reference_key_at_its_real_shape(gpu, vec):
    """The reveal key of the reference (l = 7, m = 4869, h_query of 8191 points) over a stand-in R1CS of the real shape (8185
    constraints, n = 8192), batch 2: A, B and C equal the frozen restatement.  This proof CANNOT verify -- the matrices are not the
    reveal circuit's, which exists only as Rust code; the case is here for the real columns' infinities, duplicates and opposite pairs in
    all four base sets, and for the real domain size."""
    key = gr.load_real_key()
    sy = gc.real_system()
    n, l, nc, m = gc.REAL
    assert (len(key.a_query), len(key.h_query), len(key.l_query)) == (m, n - 1, m - l)
    assert sum(p is None for p in key.a_query) > 100 and sum(p is None for p in key.b_g2_query) == 775
    zs = np.stack([oc.fr_from_ints(gc.witness(sy, k)) for k in range(2)])
    rs = [gc.blinds("real-shape", k) for k in range(2)]
    with gpu.Groth16Key.from_arrays(**gr.key_arrays(key, m, l, nc, sy.matrices())) as dk:
        assert dk.domain == n
        got = dk.prove(zs, oc.fr_from_ints([r for r, _ in rs]), oc.fr_from_ints([s for _, s in rs]))
    assert np.array_equal(got, vec["real_proofs"])


def test_key_lifecycle(gpu, vec):
    """two keys alive at once; release; use after release is an error; batch 0 and z[0] != 1 are refused; uzk_shutdown with a key left"""
    from uzkge_amd import UzkgeError, _native as N
    a, b = _key(gpu, vec, "d8_full"), _key(gpu, vec, "d64_full")
    try:
        assert a.handle != b.handle and (a.domain, b.domain) == (8, 64)
        for key, name in ((a, "d8_full"), (b, "d64_full"), (a, "d8_full")):
            assert np.array_equal(key.prove(vec[f"{name}_z"][:1], vec[f"{name}_r"][:1], vec[f"{name}_s"][:1])[0], vec[f"{name}_proofs"][0])
        z, r, s = vec["d8_full_z"][:1].copy(), vec["d8_full_r"][:1], vec["d8_full_s"][:1]
        with pytest.raises(UzkgeError) as e:
            a.prove(z[:0], r[:0], s[:0])
        assert e.value.kind == "ParameterError"
        z[0, 0] = oc.fr_from_ints([2])[0]
        with pytest.raises(UzkgeError) as e:
            a.prove(z, r, s)
        assert e.value.kind == "ParameterError"
        handle = a.handle
        a.release()
        out = np.zeros(32, dtype=np.uint64)
        zz = np.ascontiguousarray(vec["d8_full_z"][0])
        args = (zz.ctypes.data_as(ctypes.c_void_p), r.ctypes.data_as(ctypes.c_void_p), s.ctypes.data_as(ctypes.c_void_p), 1, out.ctypes.data_as(ctypes.c_void_p))
        assert N.lib.uzk_g16_prove_batch(handle, *args) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_g16_key_info(handle, None, None, None, None, None) == N.UZK_ERR_PARAMETER
        assert N.lib.uzk_g16_key_release(handle) == N.UZK_ERR_PARAMETER
        assert np.array_equal(b.prove(vec["d64_full_z"][:1], vec["d64_full_r"][:1], vec["d64_full_s"][:1])[0], vec["d64_full_proofs"][0])
        left = b.handle
        gpu.shutdown()                       # frees the key that is left
        b.handle = 0
        assert N.lib.uzk_g16_key_info(left, None, None, None, None, None) == N.UZK_ERR_PARAMETER
    finally:
        gpu.init(0)
        a.release()
        b.release()
    with _key(gpu, vec, "d8_half") as c:     # the library works again
        assert np.array_equal(c.prove(vec["d8_half_z"], vec["d8_half_r"], vec["d8_half_s"]), vec["d8_half_proofs"])
