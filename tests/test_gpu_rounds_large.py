"""The five prover rounds at the sizes where their kernels change, up to the largest circuit the library accepts.

  2^16   the last size of the lanes' one-launch grand product (z_poly_lanes) and the last size at which provers are shared
  2^17   the first size past it: round 2 runs every lane through the two-level scans of uzk_z_poly_device
  2^18   n + 3 coefficients exceed the 2^18 the lane evaluation kernel's lazy-limb sums are proven for
         (tests/test_gpu_lane_bounds.py): round 4 evaluates through the pointer-list path of uzk_poly_eval_ptrs_device
  2^20   = 2^UZK_PROVER_MAX_LOG2, the largest circuit uzk_circuit_create / uzk_prover_create accept: n + 3 coefficients are more
         than 256 blocks of 4096, so round 5 divides with 32 coefficients per lane (open_div_lanes)

tests/chain_oracle.py walks Python integers and is too slow here, so the rounds are held to the C oracle piece by piece, on the
buffers the prover shows (uzk_prover_buffer): commitments by the oracle's Pippenger over the same bases, z by the oracle's z_poly
and inverse transform, the 19 evaluations by the oracle's Horner over the downloaded coefficient polynomials and the caller's
table polynomials, both opening quotients by the oracle's division of the downloaded stack.  Every comparison is on exact field
elements and curve points: bytes are equal or the test fails.

The circuit is synthetic (random table polynomials, a random permutation of the 5n slots -- no witness satisfies it, round 3 reads
t at its expected length as tests/chain_oracle.py does); the commit bases are n + 6 valid curve points made on the device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import bn254_py as opy
import oracle_c as oc
from util import affine_of, rand_fr_wire

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from test_gpu_circuit_rounds import _run_rounds      # noqa: E402

MAX_LOG2 = 20                       # == UZK_PROVER_MAX_LOG2 (test_the_accepted_bound_is_the_tested_bound ties the two)
SIZES = [16, 17, 18]
SLOT_PI, SLOT_Z = 8, 9              # slots of a proof's own polynomials: w0..4, w_sel0..2, pi, z


def _lane(n, seed):
    """One proof's inputs, as the lane() helper of test_small_circuits_are_self_consistent makes them."""
    import prover_chain as pch
    x = pch.ChainInputs.__new__(pch.ChainInputs)
    x.n, x.m, x.seed = n, 6 * n, seed
    x.w_evals = rand_fr_wire(5 * n, seed).reshape(5, n, 4)
    x.wsel_evals = rand_fr_wire(3 * n, seed + 1).reshape(3, n, 4)
    x.pi_evals = np.zeros((n, 4), dtype=np.uint64); x.pi_evals[:8] = rand_fr_wire(8, seed + 2)
    sc = rand_fr_wire(16, seed + 3)
    x.beta, x.gamma, x.alpha, x.zeta, x.alpha_open, x.alpha_open2 = sc[0], sc[1], sc[2], sc[3], sc[4], sc[5]
    x.blinds_w = rand_fr_wire(15, seed + 4).reshape(5, 3, 4); x.blinds_w[3:, 2] = 0
    x.blinds_wsel = rand_fr_wire(9, seed + 5).reshape(3, 3, 4); x.blinds_wsel[:, 2] = 0
    x.blinds_z, x.t_rands, x.r_scalars = rand_fr_wire(3, seed + 6), rand_fr_wire(5, seed + 7), rand_fr_wire(43, seed + 8)
    return x


class Case:
    """One size: inputs made once, the circuit resident, and ONE single proof of lane 0 with the buffers the checks read."""

    def __init__(self, b, log2, lanes):
        import prover_chain as pch
        n = self.n = 1 << log2
        self.b = b
        rng = np.random.default_rng(log2)
        self.lanes = [_lane(n, 100 * (i + 1) + log2) for i in range(lanes)]
        d = b.dev_alloc((n + 6) * 64)
        try:
            b.synth_points_random(d, n + 6, 7 + log2)
            self.bases = b.dev_download(d, (n + 6, 8))
        finally:
            b.dev_free(d)
        self.perm = rng.permutation(5 * n).astype(np.uint32)
        self.k = rand_fr_wire(5, 9)
        self.polys = [rand_fr_wire(n, 300 + i) for i in range(pch.N_TABLES)]
        g = rand_fr_wire(1, 10)[0]
        self.cir = b.Circuit(n, self.bases[:n], self.bases[n:], self.perm, self.k, g, oc.fr_inv(g), rand_fr_wire(1, 11)[0], self.polys,
                             precompute=0, synthetic=True)
        self.omega = b.domain_group_gen(n)
        p = b.Prover(n, 1, shared=False)
        try:
            self.single = [_run_rounds(b, self.cir, p, [self.lanes[0]])]
            self.cs = p.buffer(b.PB_Q)[1] // 2
            hid = list(pch.HIDE_W) + [pch.HIDE_WSEL] * 3 + [0, pch.HIDE_Z]
            self.z_evals = self._slice(p, b.PB_EVALS, SLOT_Z * n, n)
            self.coefs = {s: self._slice(p, b.PB_COEFS, s * 6 * n, n + 3) for s in (0, 1, 2, 3, 4, 5, 6, 7, SLOT_Z)}
            self.hiding = hid
            self.r = self._slice(p, b.PB_R, 0, n + 3)
            self.q = [self._slice(p, b.PB_Q, w * self.cs, n + 3) for w in range(2)]
            for lane in self.lanes[1:]:
                self.single.append(_run_rounds(b, self.cir, p, [lane]))
        except BaseException:
            self.cir.release()
            raise
        finally:
            p.destroy()

    def _slice(self, prover, which, first, count):
        ptr, _ = prover.buffer(which)
        return self.b.dev_download(ptr + 32 * first, (count, 4))

    def release(self):
        self.cir.release()

    # ---- what the oracle says ------------------------------------------------------------------------------------------------
    def mono_pts(self):
        """apply_blind_factors' six bases in chain_oracle.commit_with_blinds' indexing: powers 0..2 and n..n+2."""
        n = self.n
        pts = {i: opy.wire_to_affine(self.bases[n + i].tobytes()) for i in range(3)}
        pts.update({n + i: opy.wire_to_affine(self.bases[n + 3 + i].tobytes()) for i in range(3)})
        return pts

    def group(self):
        """omega^i, i < n: the forward transform of the polynomial X."""
        x = np.zeros((self.n, 4), dtype=np.uint64)
        x[1] = oc.fr_from_ints([1])[0]
        return oc.ntt(x, threads=4)

    def hidden(self, evals, blinds):
        """add_blinds(intt(evals), blinds) of tests/chain_oracle.py in wire format: n + 3 coefficients."""
        n = self.n
        c = np.zeros((n + 3, 4), dtype=np.uint64)
        c[:n] = oc.ntt(np.ascontiguousarray(evals), inverse=True, threads=4)
        zero = np.zeros(4, dtype=np.uint64)
        for i, bl in enumerate(np.asarray(blinds).reshape(-1, 4)):
            c[i] = oc.fr_add(c[i], bl)
            c[n + i] = oc.fr_sub(zero, bl)
        return c

    def poly(self, kind, idx):
        n = self.n
        if kind == "c":
            return self.coefs[idx]
        out = np.zeros((n + 3, 4), dtype=np.uint64)
        if kind == "t":
            out[:n] = self.polys[idx]
        else:
            out[:] = self.r
        return out


_cases = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    for c in _cases.values():
        c.release()
    _cases.clear()


def case_of(gpu, log2):
    if log2 not in _cases:
        _cases[log2] = Case(gpu, log2, lanes=2 if log2 < 18 else 1)       # a lane takes 150 n x 32 bytes: one lane from 2^18 on
    return _cases[log2]


# ---- the checks, shared with the bound test --------------------------------------------------------------------------------------
def check_z(c):
    """The grand product the device holds is the oracle's, and slot z's coefficients are its hidden inverse transform."""
    x = c.lanes[0]
    z = oc.z_poly(x.w_evals, c.perm.reshape(5, c.n), c.group(), c.k, x.beta, x.gamma)
    assert np.array_equal(c.z_evals, z)
    assert np.array_equal(c.coefs[SLOT_Z], c.hidden(z, x.blinds_z))
    return z


def check_commitments(c, z, which=(0, 7)):
    import chain_oracle as co
    x, n = c.lanes[0], c.n
    o = c.single[0]
    lag, mono = np.ascontiguousarray(c.bases[:n]), c.mono_pts()
    assert affine_of(o["cm_z"][0]) == co.commit_with_blinds(lag, mono, z, oc.fr_to_ints(x.blinds_z), n)
    evals8 = [x.w_evals[i] for i in range(5)] + [x.wsel_evals[i] for i in range(3)]
    blinds8 = [x.blinds_w[i] for i in range(5)] + [x.blinds_wsel[i] for i in range(3)]
    for i in which:
        bl = oc.fr_to_ints(blinds8[i])[: c.hiding[i]]
        assert affine_of(o["cm1"][i]) == co.commit_with_blinds(lag, mono, np.ascontiguousarray(evals8[i]), bl, n), i


def check_evaluations(c):
    import prover_chain as pch
    x = c.lanes[0]
    # the coefficient polynomials the evaluations are taken of are themselves the oracle's, for one of them
    assert np.array_equal(c.coefs[0], c.hidden(x.w_evals[0], x.blinds_w[0]))
    points = (x.zeta, oc.fr_mul(x.zeta, c.omega))
    got = c.single[0]["evals"]
    plan = pch.eval_plan(True)
    assert got.shape == (len(plan), 4) and len(plan) == 19
    for i, (kind, idx, pt) in enumerate(plan):
        p = c.coefs[idx] if kind == "c" else np.ascontiguousarray(c.polys[idx])
        assert np.array_equal(got[i], oc.poly_eval(p, points[pt]).reshape(4)), (i, kind, idx, pt)


# ---- whole proofs at 2^16, 2^17, 2^18 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2", SIZES)
def test_z_and_the_round_1_and_2_commitments(gpu, log2):
    c = case_of(gpu, log2)
    check_commitments(c, check_z(c))


@pytest.mark.parametrize("log2", SIZES)
def test_round_4_evaluations_are_the_oracles_horner_values(gpu, log2):
    check_evaluations(case_of(gpu, log2))


@pytest.mark.parametrize("log2", SIZES)
def test_round_5_quotients_are_the_oracles_division(gpu, log2):
    check_quotients(case_of(gpu, log2))


def check_quotients(c):
    import prover_chain as pch
    x, n = c.lanes[0], c.n
    points = (x.zeta, oc.fr_mul(x.zeta, c.omega))
    for w, (plan, alpha) in enumerate(zip(pch.open_plan(True), (x.alpha_open, x.alpha_open2))):
        stack = np.stack([c.poly(kind, idx) for kind, idx in plan])
        q, _, _ = oc.open_quotient(stack, points[w], alpha)
        assert q[n + 1].any() and not q[n + 2].any()                          # degree n + 1
        assert np.array_equal(c.q[w], q), w


@pytest.mark.parametrize("log2", [s for s in SIZES if s < 18])
def test_a_lockstep_pair_equals_two_single_proofs(gpu, log2):
    c = case_of(gpu, log2)
    p2 = gpu.Prover(c.n, 2)
    try:
        o2 = _run_rounds(gpu, c.cir, p2, c.lanes)
    finally:
        p2.destroy()
    for i, o1 in enumerate(c.single):
        for key, per in (("cm1", 8), ("cm_z", 1), ("cm_t", 5), ("cm_q", 2)):
            assert [affine_of(j) for j in o2[key][i * per:(i + 1) * per]] == [affine_of(j) for j in o1[key]], (log2, i, key)
        assert np.array_equal(o2["evals"][i * 19:(i + 1) * 19], o1["evals"]), (log2, i)


def test_a_zero_denominator_past_the_lane_scan_still_names_its_proof(gpu):
    """n = 2^17: round 2 runs the lanes one by one through uzk_z_poly_device; the lane whose gamma makes a denominator zero is
    refused by number, first and last, and the prover goes on to make both proofs with their own challenges."""
    from types import SimpleNamespace

    from test_gpu_zero_denominator_rounds import _round1, poisoned
    from uzkge_amd import UzkgeError
    from uzkge_amd import _native as N
    c = case_of(gpu, 17)
    cir_inp = SimpleNamespace(perm=c.perm, k=c.k, group_gen=c.omega)
    cat = lambda f, ls: np.concatenate([np.ascontiguousarray(f(x), dtype=np.uint64).reshape(-1, 4) for x in ls])
    p2 = gpu.Prover(c.n, 2, shared=False)
    try:
        for bad in (1, 0):
            _round1(p2, c.cir, c.lanes)
            ls = [poisoned(x, cir_inp) if i == bad else x for i, x in enumerate(c.lanes)]
            with pytest.raises(UzkgeError) as e:
                p2.round2(cat(lambda x: x.beta, ls), cat(lambda x: x.gamma, ls), cat(lambda x: x.blinds_z, ls))
            assert e.value.code == N.UZK_ERR_PARAMETER and f"proof {bad}:" in str(e.value) and "denominator" in str(e.value), (bad, str(e.value))
        _round1(p2, c.cir, c.lanes)
        cm_z = p2.round2(cat(lambda x: x.beta, c.lanes), cat(lambda x: x.gamma, c.lanes), cat(lambda x: x.blinds_z, c.lanes))
        assert [affine_of(j) for j in cm_z] == [affine_of(o["cm_z"][0]) for o in c.single]
    finally:
        p2.destroy()


# ---- the accepted bound is the tested bound -----------------------------------------------------------------------------------------
def test_the_accepted_bound_is_the_tested_bound(gpu):
    """The largest n uzk_circuit_create and uzk_prover_create[_private] accept is a size at which this module makes a whole proof
    (all five rounds, one lane) and holds z, cm_z, the evaluations and -- the division runs its widest kernel only here -- the
    opening quotients to the oracle; one size further is refused at creation, by all three, and never in a later round."""
    from uzkge_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "uzkge_gpu.h")).read()
    assert int(re.search(r"#define UZK_PROVER_MAX_LOG2 (\d+)", hdr).group(1)) == MAX_LOG2
    c = case_of(gpu, MAX_LOG2)
    assert set(c.single[0]) == {"cm1", "cm_z", "cm_t", "evals", "cm_q"} and c.single[0]["cm_q"].shape == (2, 12)
    check_commitments(c, check_z(c), which=())
    check_evaluations(c)
    check_quotients(c)
    h = ctypes.c_uint64(0)
    for create in (N.lib.uzk_prover_create, N.lib.uzk_prover_create_private):
        assert create(2 << MAX_LOG2, 1, ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    d = N.CircuitDesc(); d.n = 2 << MAX_LOG2
    assert N.lib.uzk_circuit_create(ctypes.byref(d), ctypes.byref(h)) == N.UZK_ERR_PARAMETER
    assert f"2^{MAX_LOG2}" in N.lib.uzk_last_error().decode()
