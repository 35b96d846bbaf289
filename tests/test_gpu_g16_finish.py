"""The Groth16 prover that ends on the device (uzk_g16_prove_batch_finish; Groth16Key.prove(..., finish="device")): the frozen proofs of
tests/golden/vectors_g16.npz through the new entry, a batch across the group of 128, the reference key's real columns, the blob
against its definition written out in Python integers, the finish kernels alone (uzk_test_g16_finish) on points k G of known k in
every degenerate branch, and the refusals.  Every comparison is bit-exact on canonical words."""
import ctypes
import os
import random

import numpy as np
import pytest

import bn254_py as opy
import g16_cases as gc
import g16_ref as gr
import oracle_c as oc

pytestmark = pytest.mark.gpu

NAMES = tuple(gc.CASES)
P, R = opy.P, opy.R
G = (1, 2)


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


def blob_of(proof) -> bytes:
    """the blob of uzk_g16_verify_batch from one [32]-word proof (A 8 words, B 16, C 8; Montgomery): a.x, a.y, b.x.c1, b.x.c0, b.y.c1,
    b.y.c0, c.x, c.y, each the canonical integer in 32 big-endian bytes"""
    w = [opy.from_mont(sum(int(proof[4 * k + j]) << (64 * j) for j in range(4)), P) for k in range(8)]
    ax, ay, bx0, bx1, by0, by1, cx, cy = w
    return b"".join(v.to_bytes(32, "big") for v in (ax, ay, bx1, bx0, by1, by0, cx, cy))


def check_blobs(proofs, blobs):
    assert blobs.shape == (proofs.shape[0], 256) and blobs.dtype == np.uint8
    for b in range(proofs.shape[0]):
        assert bytes(blobs[b]) == blob_of(proofs[b]), b


@pytest.mark.parametrize("name", NAMES)
def test_frozen_proofs_through_the_device_finish(gpu, vec, name):
    """batch 1 and 3 against the frozen proofs; r = s = 0 (both chains return infinity, C = K) and r = s = r_mod - 1; the
    device-assignment form against the host form; every blob against its definition"""
    with _key(gpu, vec, name) as key:
        z, r, s = vec[f"{name}_z"], vec[f"{name}_r"], vec[f"{name}_s"]
        want = vec[f"{name}_proofs"]
        p1, b1 = key.prove(z[:1], r[:1], s[:1], finish="device")
        assert p1.shape == (1, 32) and np.array_equal(p1[0], want[0])
        check_blobs(p1, b1)
        got, blobs = key.prove(z, r, s, finish="device")
        for b in range(gc.BATCH):
            assert np.array_equal(got[b], want[b]), b
        check_blobs(got, blobs)
        zero, rm1 = oc.fr_from_ints([0]), oc.fr_from_ints([gr.R - 1])
        pz, bz = key.prove(z[:1], zero, zero, finish="device")
        assert np.array_equal(pz[0], vec[f"{name}_proof_zero"])
        check_blobs(pz, bz)
        pm, bm = key.prove(z[:1], rm1, rm1, finish="device")
        assert np.array_equal(pm[0], vec[f"{name}_proof_rm1"])
        check_blobs(pm, bm)
        d = gpu.dev_alloc(z.nbytes)
        d_blobs = gpu.dev_alloc(gc.BATCH * 256)
        try:
            gpu.dev_upload(d, z)
            pd, bd = key.prove_device(d, r, s, finish="device", d_blobs=d_blobs)
            assert np.array_equal(pd, want) and np.array_equal(bd, blobs)
            left = gpu.dev_download(d_blobs, (gc.BATCH * 32,))            # the blobs left on the device, as words
            assert left.tobytes() == blobs.tobytes()
        finally:
            gpu.dev_free(d)
            gpu.dev_free(d_blobs)


def test_batch_across_the_group_boundary(gpu, vec):
    """batch 129 at domain 8: the second group holds one proof.  Proofs 0, 127 and 128 equal the closed form of the trapdoor key; all 129
    equal the host finish (the existing entry) called here"""
    name = "d8_full"
    sy, trap = gc.case_system(name), gc.trapdoor(name)
    zs = [gc.witness(sy, k) for k in range(gc.BIG_BATCH)]
    rs = [gc.blinds(name, k) for k in range(gc.BIG_BATCH)]
    z, r, s = np.stack([oc.fr_from_ints(z) for z in zs]), oc.fr_from_ints([r for r, _ in rs]), oc.fr_from_ints([s for _, s in rs])
    with _key(gpu, vec, name) as key:
        got, blobs = key.prove(z, r, s, finish="device")
        host = key.prove(z, r, s)
    assert got.shape == (gc.BIG_BATCH, 32)
    for b in (0, 127, 128):
        h = gr.witness_map(sy.matrices(), sy.l, zs[b])
        want = gr.proof_to_wire(gr.points_of(*gr.closed_form(sy.matrices(), sy.l, zs[b], rs[b][0], rs[b][1], trap, h)))
        assert want.any() and np.array_equal(got[b], want), b
    for b in range(gc.BIG_BATCH):
        assert np.array_equal(got[b], host[b]), b
    check_blobs(got, blobs)


def test_the_reference_key_at_its_real_shape(gpu, vec):
    """the reveal key of the reference over the stand-in R1CS of the real shape, batch 2: b_g2_query's 775 infinities, its duplicates and
    its opposite pairs in front of the device Horner chain"""
    key = gr.load_real_key()
    sy = gc.real_system()
    n, l, nc, m = gc.REAL
    assert sum(p is None for p in key.b_g2_query) == 775
    zs = np.stack([oc.fr_from_ints(gc.witness(sy, k)) for k in range(2)])
    rs = [gc.blinds("real-shape", k) for k in range(2)]
    with gpu.Groth16Key.from_arrays(**gr.key_arrays(key, m, l, nc, sy.matrices())) as dk:
        assert dk.domain == n
        got, blobs = dk.prove(zs, oc.fr_from_ints([r for r, _ in rs]), oc.fr_from_ints([s for _, s in rs]), finish="device")
    assert np.array_equal(got, vec["real_proofs"])
    check_blobs(got, blobs)


# ---- the finish kernels alone --------------------------------------------------------------------------------------------------------
def _fq_words(xs):
    return oc.fr_from_ints(xs, mod=P)


def _jac(k, zc=1):
    """the Jacobian words of k G with Z = zc (k = 0 mod r: infinity, z = 0 with x, y arbitrary)"""
    if k % R == 0:
        return _fq_words([zc % P or 1, 5, 0]).reshape(12)
    x, y = opy.g1_mul(G, k % R)
    return _fq_words([x * zc * zc % P, y * pow(zc, 3, P) % P, zc % P]).reshape(12)


def _aff_words(k):
    return oc.points_from_affine([opy.g1_mul(G, k % R) if k % R else (0, 0)])[0]


def _finish(a, b1, kk, r, s):
    """uzk_test_g16_finish on lists of 12-word Jacobian points and integer blinds -> (a_out [n, 8], c_out [n, 8])"""
    from uzkge_amd import _native as N
    from uzkge_amd.errors import check
    n = len(a)
    arr = lambda rows: np.ascontiguousarray(np.stack(rows), dtype=np.uint64)
    A, B1, K = arr(a), arr(b1), arr(kk)
    rw, sw = oc.fr_from_ints(r), oc.fr_from_ints(s)
    a_out, c_out = np.full((n, 8), 0xdead, dtype=np.uint64), np.full((n, 8), 0xdead, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    check(N.lib.uzk_test_g16_finish(p(A), p(B1), p(K), p(rw), p(sw), n, p(a_out), p(c_out)))
    return a_out, c_out


def test_the_finish_kernels_in_every_branch(gpu):
    """records (a, b1, k, r, s) with A = a G, B1 = b1 G, K = k G: the expected C is (s a + r b1 + k) G from Python integers.  65 further
    random records put the batch past one wave and the named ones on both sides of its boundary."""
    rng = random.Random("g16-finish-hook")
    rnd = lambda: rng.randrange(1, R)
    a0, s0, k0 = rnd(), rnd(), rnd()
    cases = [
        ("A = B1, s = r: the combination doubles", a0, a0, k0, s0, s0),
        ("A = -B1, s = r: the sum is infinity, C = K", a0, R - a0, k0, s0, s0),
        ("K = -(s A + r B1): C is infinity", a0, rnd(), None, rnd(), rnd()),
        ("A infinite", 0, rnd(), rnd(), rnd(), rnd()),
        ("B1 infinite", rnd(), 0, rnd(), rnd(), rnd()),
        ("K infinite", rnd(), rnd(), 0, rnd(), rnd()),
        ("all three infinite", 0, 0, 0, rnd(), rnd()),
        ("s = 1, r = 1", rnd(), rnd(), rnd(), 1, 1),
        ("s = r = r_mod - 1", rnd(), rnd(), rnd(), R - 1, R - 1),
        ("s = r = 0: C = K", rnd(), rnd(), rnd(), 0, 0),
        ("the doubling with K infinite", a0, a0, 0, s0, s0),
        ("the cancellation with K infinite: C is infinity", a0, R - a0, 0, s0, s0),
    ]
    recs = []
    for what, a, b1, k, r, s in cases:
        if k is None:
            k = -(s * a + r * b1) % R
        recs.append((what, a, b1, k, r, s, 1, 1, 1))
    # Z != 1, and one record twice under different Z: the outputs must be equal
    a1, b11, k1, r1, s1 = rnd(), rnd(), rnd(), rnd(), rnd()
    recs.append(("Z != 1 (first)", a1, b11, k1, r1, s1, rng.randrange(2, P), rng.randrange(2, P), rng.randrange(2, P)))
    recs.append(("Z != 1 (second)", a1, b11, k1, r1, s1, rng.randrange(2, P), P - 1, 2))
    named = len(recs)
    for i in range(65):
        recs.append((f"random {i}", rnd(), rnd(), rnd(), rnd(), rnd(), rng.randrange(1, P), rng.randrange(1, P), rng.randrange(1, P)))
    recs = recs[:3] + recs[named:named + 60] + recs[3:named] + recs[named + 60:]           # named records at lanes 0..2 and 63..
    a_out, c_out = _finish([_jac(a, za) for _, a, _, _, _, _, za, _, _ in recs], [_jac(b1, zb) for _, _, b1, _, _, _, _, zb, _ in recs],
                           [_jac(k, zk) for _, _, _, k, _, _, _, _, zk in recs], [r for _, _, _, _, r, _, _, _, _ in recs], [s for _, _, _, _, _, s, _, _, _ in recs])
    seen = {}
    for i, (what, a, b1, k, r, s, *_z) in enumerate(recs):
        c = (s * a + r * b1 + k) % R
        assert np.array_equal(a_out[i], _aff_words(a)), what
        assert np.array_equal(c_out[i], _aff_words(c)), what
        if "infinity" in what and "C is" in what:
            assert c == 0 and not c_out[i].any(), what
        if what.startswith("Z != 1"):
            seen[what] = (a_out[i].copy(), c_out[i].copy())
    assert np.array_equal(seen["Z != 1 (first)"][0], seen["Z != 1 (second)"][0]) and np.array_equal(seen["Z != 1 (first)"][1], seen["Z != 1 (second)"][1])
    assert seen["Z != 1 (first)"][1].any()


def test_refusals(gpu, vec):
    """both outputs NULL, batch 0, z[0] != 1 and a released key are UZK_ERR_PARAMETER"""
    from uzkge_amd import UzkgeError, _native as N
    name = "d8_full"
    key = _key(gpu, vec, name)
    try:
        z, r, s = np.ascontiguousarray(vec[f"{name}_z"][:1]).copy(), np.ascontiguousarray(vec[f"{name}_r"][:1]), np.ascontiguousarray(vec[f"{name}_s"][:1])
        p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        out, blobs = np.zeros(32, dtype=np.uint64), np.zeros(256, dtype=np.uint8)
        fin = N.lib.uzk_g16_prove_batch_finish
        assert fin(key.handle, p(z), 0, p(r), p(s), 1, None, None, None) == N.UZK_ERR_PARAMETER
        assert fin(key.handle, p(z), 0, p(r), p(s), 0, p(out), p(blobs), None) == N.UZK_ERR_PARAMETER
        with pytest.raises(UzkgeError) as e:
            key.prove(z[:0], r[:0], s[:0], finish="device")
        assert e.value.kind == "ParameterError"
        assert fin(key.handle, p(z), 0, p(r), p(s), 1, p(out), None, None) == N.UZK_OK                  # one output is enough
        assert np.array_equal(out, vec[f"{name}_proofs"][0])
        assert fin(key.handle, p(z), 0, p(r), p(s), 1, None, p(blobs), None) == N.UZK_OK
        assert bytes(blobs) == blob_of(out)
        bad = z.copy()
        bad[0, 0] = oc.fr_from_ints([2])[0]
        with pytest.raises(UzkgeError) as e:
            key.prove(bad, r, s, finish="device")
        assert e.value.kind == "ParameterError"
        with pytest.raises(ValueError):
            key.prove(z, r, s, finish="gpu")
        handle = key.handle
        key.release()
        assert fin(handle, p(z), 0, p(r), p(s), 1, p(out), p(blobs), None) == N.UZK_ERR_PARAMETER
    finally:
        key.release()
