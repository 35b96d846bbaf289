"""CPU checks of the Groth16 restatement (tests/g16_ref.py) and of the argument validation of uzk_g16_key_create: the key fixtures and
their section lengths, the frozen vectors of tests/golden/vectors_g16.npz, h Z = a b - c at a random point, the closed form of a
trapdoor proof, the verifier equation, and the descriptor checks that run before the device is touched."""
import ctypes
import os
import random
import struct

import numpy as np
import pytest

import g16_cases as gc
import g16_ref as gr
import g2_ref as g2
import oracle_c as oc

R = gr.R
SMALL = ("d8_full", "d8_half", "d64_full", "d64_half")


@pytest.fixture(scope="module")
def vec(golden_dir):
    return np.load(os.path.join(golden_dir, "vectors_g16.npz"))


def test_fixture_hashes_and_section_lengths():
    assert gr.sha256_of(gr.HEAD) == gr.HEAD_SHA256 and gr.sha256_of(gr.TAIL) == gr.TAIL_SHA256
    assert gr.sha256_of(g2.FIXTURE) == g2.FIXTURE_SHA256
    data = open(gr.HEAD, "rb").read() + open(g2.FIXTURE, "rb").read() + open(gr.TAIL, "rb").read()
    assert len(data) == 1041488
    pos, lens = 32 + 3 * 64, []
    for width, skip in ((32, 64), (32, 0), (32, 0), (64, 0), (32, 0), (32, 0)):      # beta_g1 and delta_g1 follow gamma_abc_g1
        n = struct.unpack_from("<Q", data, pos)[0]
        lens.append(n)
        pos += 8 + n * width + skip
    assert tuple(lens) == gr.SECTION_LENS == (7, 4869, 4869, 4869, 8191, 4862) and pos == len(data)
    key = gr.load_real_key()
    assert tuple(len(getattr(key, f)) for f in ("gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")) == gr.SECTION_LENS
    assert gc.REAL == (8192, 7, 8185, 4869) and gr.domain_of(8185, 7) == 8192


@pytest.mark.parametrize("name", tuple(gc.CASES))
def test_the_generator_and_the_witness_map_reproduce_the_npz(vec, name):
    """matrices, assignments, blinds, h (satisfying and not) as frozen; the frozen key's points for the small domains"""
    sy = gc.case_system(name)
    n, l, nc = gc.CASES[name][:3]
    assert (sy.n, sy.l, sy.nc) == (n, l, nc) and gr.domain_of(nc, l) == n and nc + l in (n, n // 2 + 1)
    for tag, M in zip("ABC", sy.matrices()):
        ptr, col, val = gr.csr(M)
        assert np.array_equal(ptr, vec[f"{name}_{tag}_ptr"]) and np.array_equal(col, vec[f"{name}_{tag}_col"])
        assert np.array_equal(val, vec[f"{name}_{tag}_val"].reshape(-1, 4))
        assert gr.from_csr(ptr, col, val) == M
    zs = [gc.witness(sy, k) for k in range(gc.BATCH)]
    assert np.array_equal(np.stack([oc.fr_from_ints(z) for z in zs]), vec[f"{name}_z"])
    rs = [gc.blinds(name, k) for k in range(gc.BATCH)]
    assert np.array_equal(oc.fr_from_ints([r for r, _ in rs]), vec[f"{name}_r"]) and np.array_equal(oc.fr_from_ints([s for _, s in rs]), vec[f"{name}_s"])
    assert np.array_equal(oc.fr_from_ints(gr.witness_map(sy.matrices(), l, zs[0])), vec[f"{name}_h"])
    zb = oc.fr_to_ints(vec[f"{name}_z_bad"])
    assert not gc.satisfied(sy, zb) and sum(x != y for x, y in zip(zb, zs[0])) == 1
    assert np.array_equal(oc.fr_from_ints(gr.witness_map(sy.matrices(), l, zb)), vec[f"{name}_h_bad"])
    if name in SMALL[:2]:
        key = gr.trapdoor_setup(sy.matrices(), l, sy.m, gc.trapdoor(name))
        for f in ("a_query", "b_g1_query", "h_query", "l_query", "gamma_abc_g1"):
            assert np.array_equal(gr.g1_to_wire(getattr(key, f)), vec[f"{name}_{f}"]), f
        assert np.array_equal(g2.points_to_wire(key.b_g2_query), vec[f"{name}_b_g2_query"])
        assert key.a_query[-1] is None and key.b_g2_query[-1] is None and key.l_query[-1] is None      # the variable no row mentions


def test_row_shapes_of_the_cases():
    """an empty row, rows of one entry, one of 254 entries, rows at and beyond the kernel's slice length, an unused variable"""
    for name in ("d64_full", "d64_half", "d1024_full", "d1024_half"):
        sy = gc.case_system(name)
        lens = [len(r) for r in sy.A]
        for want in (0, 1, 254, gc.SLICE, gc.SLICE + 1, gc.SLICE + 8):
            assert want in lens, (name, want)
        used = {c for M in sy.matrices() for r in M for c, _ in r}
        assert sy.m - 1 not in used
    for name in SMALL[:2]:
        sy = gc.case_system(name)
        assert 0 in [len(r) for r in sy.A] and 0 in [len(r) for r in sy.C]


@pytest.mark.parametrize("name", tuple(gc.CASES))
def test_h_times_z_is_ab_minus_c_at_a_random_point(name):
    """for every satisfying assignment h(x) Z(x) = a(x) b(x) - c(x) with a, b, c the interpolants over the domain, and h[n - 1] = 0"""
    sy = gc.case_system(name)
    rng = random.Random(f"g16-point-{name}")
    for k in range(gc.BATCH):
        z = gc.witness(sy, k)
        assert gc.satisfied(sy, z)
        h = gr.witness_map(sy.matrices(), sy.l, z)
        assert len(h) == sy.n and h[-1] == 0
        x = rng.randrange(R)
        L = gr.lagrange_at(sy.n, x)
        a = sum(gc.dot(r, z) * L[i] for i, r in enumerate(sy.A)) + sum(z[j] * L[sy.nc + j] for j in range(sy.l))
        b = sum(gc.dot(r, z) * L[i] for i, r in enumerate(sy.B))
        c = sum(gc.dot(r, z) * L[i] for i, r in enumerate(sy.C))
        hx = sum(v * pow(x, i, R) for i, v in enumerate(h))
        assert hx * (pow(x, sy.n, R) - 1) % R == (a * b - c) % R


def _frozen_key(vec, name):
    g1 = lambda f: gr.g1_from_wire(vec[f"{name}_{f}"])
    p2 = lambda f: [g2.point_from_wire(w) for w in vec[f"{name}_{f}"].reshape(-1, 16)]
    return gr.Key(alpha_g1=g1("alpha_g1")[0], beta_g1=g1("beta_g1")[0], delta_g1=g1("delta_g1")[0], beta_g2=p2("beta_g2")[0], gamma_g2=p2("gamma_g2")[0],
                  delta_g2=p2("delta_g2")[0], gamma_abc_g1=g1("gamma_abc_g1"), a_query=g1("a_query"), b_g1_query=g1("b_g1_query"),
                  b_g2_query=p2("b_g2_query"), h_query=g1("h_query"), l_query=g1("l_query"))


@pytest.mark.parametrize("name", tuple(gc.CASES))
def test_every_trapdoor_proof_equals_the_closed_form(vec, name):
    """A = (alpha + sum z_i A_i(tau) + r delta) G, likewise B and C -- for every frozen proof; at the small domains the restatement's
    prover (MSMs over the frozen key) reproduces the frozen proofs too"""
    sy, trap = gc.case_system(name), gc.trapdoor(name)
    zs = [gc.witness(sy, k) for k in range(gc.BATCH)]
    rs = [gc.blinds(name, k) for k in range(gc.BATCH)]
    hs = [gr.witness_map(sy.matrices(), sy.l, z) for z in zs]
    for k in range(gc.BATCH):
        want = gr.proof_to_wire(gr.points_of(*gr.closed_form(sy.matrices(), sy.l, zs[k], rs[k][0], rs[k][1], trap, hs[k])))
        assert np.array_equal(want, vec[f"{name}_proofs"][k]), k
    for tag, v in (("zero", 0), ("rm1", R - 1)):
        want = gr.proof_to_wire(gr.points_of(*gr.closed_form(sy.matrices(), sy.l, zs[0], v, v, trap, hs[0])))
        assert np.array_equal(want, vec[f"{name}_proof_{tag}"]), tag
    if name in SMALL:
        key = _frozen_key(vec, name)
        assert np.array_equal(gr.proof_to_wire(gr.prove(key, sy.matrices(), sy.l, zs[1], rs[1][0], rs[1][1], hs[1])), vec[f"{name}_proofs"][1])


def test_the_verifier_equation_at_domain_8(vec):
    """e(A, B) = e(alpha, beta) e(sum z_i IC_i, gamma) e(C, delta) for a frozen proof; not for the proof of an assignment with one
    element flipped, nor for the frozen proof under other public inputs"""
    name = "d8_full"
    sy = gc.case_system(name)
    key = _frozen_key(vec, name)
    z = gc.witness(sy, 0)
    w = vec[f"{name}_proofs"][0]
    proof = (gr.g1_from_wire(w[0:8])[0], g2.point_from_wire(w[8:24]), gr.g1_from_wire(w[24:32])[0])
    assert gr.verify(key, z[:sy.l], proof)
    zb = oc.fr_to_ints(vec[f"{name}_z_bad"])
    r, s = gc.blinds(name, 0)
    assert not gr.verify(key, zb[:sy.l], gr.prove(key, sy.matrices(), sy.l, zb, r, s))
    assert not gr.verify(key, [1, (z[1] + 1) % R], proof)


def test_key_create_validates_its_descriptor_before_the_device(vec):
    """uzk_g16_key_create: every refusal below is decided on the host, with or without a GPU; without one a well-formed descriptor
    fails with DeviceError (no CPU fallback)"""
    from uzkge_amd import _native as N, backend as b
    name = "d8_full"
    n, l, nc = gc.CASES[name][:3]
    m = vec[f"{name}_a_query"].shape[0]
    mats = [(vec[f"{name}_{t}_ptr"], vec[f"{name}_{t}_col"], vec[f"{name}_{t}_val"]) for t in "ABC"]

    def create(n_vars=m, n_inputs=l, n_constraints=nc, matrices=mats, mutate=None, **over):
        cols = {f: vec[f"{name}_{f}"] for f in ("a_query", "b_g1_query", "l_query", "h_query", "b_g2_query")}
        cols.update(over)
        d, keep = b.Groth16Key.describe(n_vars, n_inputs, n_constraints, vec[f"{name}_alpha_g1"], vec[f"{name}_beta_g1"], vec[f"{name}_delta_g1"],
                                        vec[f"{name}_beta_g2"], vec[f"{name}_delta_g2"], cols["a_query"], cols["b_g1_query"], cols["l_query"],
                                        cols["h_query"], cols["b_g2_query"], matrices)
        if mutate:
            mutate(d)
        h = ctypes.c_uint64(0)
        rc = N.lib.uzk_g16_key_create(ctypes.byref(d), ctypes.byref(h))
        if rc == N.UZK_OK:
            assert N.lib.uzk_g16_key_release(h.value) == N.UZK_OK
        return rc

    def with_matrix(k, ptr=None, col=None):
        out = list(mats)
        out[k] = (mats[k][0] if ptr is None else ptr, mats[k][1] if col is None else col, mats[k][2])
        return out

    h = ctypes.c_uint64(0)
    assert N.lib.uzk_g16_key_create(None, ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    assert create(n_inputs=0) == N.UZK_ERR_PARAMETER                                   # l >= 1
    assert create(n_inputs=m + 1) == N.UZK_ERR_PARAMETER                               # l <= m
    assert create(n_constraints=0) == N.UZK_ERR_PARAMETER
    bad_ptr = mats[1][0].copy(); bad_ptr[2] = bad_ptr[3] + 1                           # row pointers decrease
    assert create(matrices=with_matrix(1, ptr=bad_ptr)) == N.UZK_ERR_PARAMETER
    bad_ptr = mats[0][0].copy(); bad_ptr[0] = 1
    assert create(matrices=with_matrix(0, ptr=bad_ptr)) == N.UZK_ERR_PARAMETER
    bad_col = mats[2][1].copy(); bad_col[-1] = m                                        # col < m
    assert create(matrices=with_matrix(2, col=bad_col)) == N.UZK_ERR_PARAMETER
    assert create(l_query=vec[f"{name}_l_query"][:-1]) == N.UZK_ERR_PARAMETER          # l_query has m - l entries
    assert create(h_query=vec[f"{name}_h_query"][:-1]) == N.UZK_ERR_PARAMETER          # h_query has n - 1 entries
    assert create(mutate=lambda d: setattr(d, "a_query", None)) == N.UZK_ERR_PARAMETER
    assert create(mutate=lambda d: d.row_ptr.__setitem__(2, None)) == N.UZK_ERR_PARAMETER
    # a domain this library does not transform over (2^26 points): refused before the matrices are read
    assert create(n_constraints=1 << 25) == N.UZK_ERR_DEGREE
    assert N.lib.uzk_g16_key_release(12345) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_g16_key_info((1 << 58) | 99, None, None, None, None, None) == N.UZK_ERR_PARAMETER
    p = np.zeros(64, dtype=np.uint64).ctypes.data_as(ctypes.c_void_p)
    assert N.lib.uzk_g16_prove_batch(12345, p, p, p, 1, p) == N.UZK_ERR_PARAMETER
    assert N.lib.uzk_g16_prove_batch(12345, p, p, p, 0, p) == N.UZK_ERR_PARAMETER       # batch == 0
    assert N.lib.uzk_g16_h_device(12345, p, 0, p) == N.UZK_ERR_PARAMETER
    rc = create()
    assert rc == (N.UZK_OK if b.device_count() > 0 else N.UZK_ERR_DEVICE)
