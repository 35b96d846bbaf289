"""The NTT's short-input path on its own, and the zero tails it relies on.

`ntt_run` (uzkge_amd/csrc/ntt.hip) takes the caller's statement `in_len`: every input vector of a forward transform over 3 * 2^k
points is zero from index in_len on.  With fused sub-transforms (m3 = n / 3 >= 4096) and 0 < in_len <= m3 the first Stockham pass
(`short_in` of ntt_pass29_kernel<B, FIRST = true, TILE>) reads neither x[j + m3] nor x[j + 2 m3], takes the radix-3 combination to be
x[j] itself, and sets every element with j >= in_len to zero WITHOUT reading it.  Only the prover says so (derive_cosets: in_len = n
on 6n-point slots; round 3: n + 8 over all coefficient slots), so every proof runs this branch and nothing else did until this file:
`uzk_test_ntt_in_len` (include/uzkge_gpu_test.h) is the public strided entry point with that one more argument.

All comparisons are byte equality of wire words.  References: the C oracle's transform of the zero-padded vector (m3 <= 2^17) and
the library's own full path (in_len = 0) on the same zero-padded input, which tests/test_gpu_ntt_large.py and
test_gpu_variants.py::test_ntt_fused_stages_match_the_oracle hold to the oracle; both where both exist.  One size per first-pass
radix of get_plan: 6 bits at k = 12, 7 at 13, 8 at 14, 9 at 17, 10 at 19, 11 at 21, and 8 bits in three passes at k = 17 with
uzk_tune("ntt_two_pass", 0); both tile instantiations at every size (the prover's 10 slots at n = 2^20 run the 2048-element tile).

The second half holds the CONTRACT at its call sites: a prover's coefficient slots are zero beyond n + 3 after rounds 1 and 2 of
every proof of a sequence on one prover, round 3's t equals the oracle chain's, and derive_cosets' tables equal the oracle's coset
FFT of full-length coefficient forms."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import oracle_c as oc
from util import GOLDEN

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

SHIFTS = (None,) + tuple(oc.fr_from_ints([7, 12345678901234567890123]))     # the fused-stage test's two coset shifts
SIZES = (12, 13, 14, 17, 19, 21)                 # n = 3 * 2^k: one per first-pass radix
ORACLE_MAX_K = 17                                # beyond: the library's full path alone (an oracle run would take the test beyond a few seconds)
BATCH = 3                                        # k = 21, batch 3: more than 2^24 points in a launch, the 2048-element tile by size
IN_LENS = ("1", "2", "255", "256", "257", "m3/2", "m3/2+8", "m3-1", "m3")
POISON = -1                                      # all-ones words: non-canonical, above the modulus
SENTINEL = 0x5E5E5E5E5E5E5E5E


def _in_len(name, m3):
    return {"m3/2": m3 // 2, "m3/2+8": m3 // 2 + 8, "m3-1": m3 - 1, "m3": m3}.get(name) or int(name)


class _Size:
    """Device buffers of one size, reused by every case of that size: x = `batch` different random canonical vectors."""

    def __init__(self, gpu, k, batch):
        self.k, self.n, self.m3, self.batch = k, 3 << k, 1 << k, batch
        n = self.n
        self.x = torch.empty((batch * n, 4), dtype=torch.int64, device="cuda")
        self.src, self.out, self.ref = (torch.empty_like(self.x) for _ in range(3))
        torch.cuda.synchronize()
        gpu.synth_scalars(self.x.data_ptr(), batch * n, 4000 + k)
        gpu.sync()
        self.xv = self.x.view(batch, n, 4)
        v = self.xv
        assert not torch.equal(v[0], v[1 % batch]) or batch == 1

    def padded(self, in_len, fill=0, batch=None):
        """src = the first `batch` vectors of x with [in_len, n) of each replaced by `fill` words; element in_len - 1 is non-zero."""
        b = self.batch if batch is None else batch
        s = self.src.view(self.batch, self.n, 4)[:b]
        s.copy_(self.xv[:b])
        assert bool((s[:, in_len - 1] != 0).any(dim=1).all())
        s[:, in_len:] = fill
        torch.cuda.synchronize()                         # torch's stream; the library runs on its own
        return s

    def oracle(self, in_len, shift, batch=None):
        b = self.batch if batch is None else batch
        h = self.xv[:b].cpu().numpy().view(np.uint64).copy()
        h[:, in_len:] = 0
        want = np.stack([oc.ntt(np.ascontiguousarray(h[i]) if shift is None else oc.mul_var(np.ascontiguousarray(h[i]), shift), threads=4)
                         for i in range(b)])
        return torch.from_numpy(want.view(np.int64)).cuda()


_state = {}


def _size(gpu, k, batch=None):
    batch = BATCH if batch is None else batch
    s = _state.get("size")
    if s is None or (s.k, s.batch) != (k, batch):
        _state.clear()
        torch.cuda.empty_cache()
        s = _state["size"] = _Size(gpu, k, batch)
    return s


@pytest.fixture(autouse=True, scope="module")
def _release_buffers():
    yield
    for d in (_state, _chain, _oracle_runs):
        d.clear()
    torch.cuda.empty_cache()


def _tunes(k):
    """(ntt_tile, ntt_two_pass): by size, both tile instantiations, and at k = 17 the three passes of 8 bits"""
    return [(0, 1), (1024, 1), (2048, 1)] + ([(0, 0), (2048, 0)] if k == 17 else [])


def _reference(gpu, S, in_len, shift, batch=None):
    """S.ref[:batch] = the transform of the clean zero-padded vectors: the library's full path, and the oracle where it is affordable."""
    b = S.batch if batch is None else batch
    src = S.padded(in_len, 0, b)
    ref = S.ref.view(S.batch, S.n, 4)[:b]
    gpu.ntt_in_len_device(src.data_ptr(), 0, ref.data_ptr(), 0, S.n, b, 0, shift)
    if S.k <= ORACLE_MAX_K:
        assert torch.equal(ref, S.oracle(in_len, shift, b)), "full path vs oracle"
    return ref


@pytest.mark.parametrize("name", IN_LENS)
@pytest.mark.parametrize("si", range(len(SHIFTS)))
@pytest.mark.parametrize("k", SIZES)
def test_short_input_path_equals_the_transform_of_the_zero_padded_vector(gpu, k, si, name):
    """Every in_len at and around the branch's edges, clean tails and poisoned ones (the tail is never read: this pins `j < in_len`
    and that the short path ran at in_len = m3), out of place and in place, every tile / pass plan of the size."""
    S, shift = _size(gpu, k), SHIFTS[si]
    n, B = S.n, S.batch
    in_len = _in_len(name, S.m3)
    try:
        ref = _reference(gpu, S, in_len, shift)
        out = S.out.view(B, n, 4)
        for fill in (0, POISON):
            for tile, two in _tunes(k):
                gpu.tune("ntt_tile", tile)
                gpu.tune("ntt_two_pass", two)
                src = S.padded(in_len, fill)
                keep = src.clone()
                out.fill_(SENTINEL)
                torch.cuda.synchronize()
                gpu.ntt_in_len_device(src.data_ptr(), 0, out.data_ptr(), 0, n, B, in_len, shift)
                assert torch.equal(out, ref), (k, name, si, fill, tile, two, "out of place")
                assert torch.equal(src, keep), "the input is not written"
                gpu.ntt_in_len_device(src.data_ptr(), 0, src.data_ptr(), 0, n, B, in_len, shift)      # as derive_cosets calls it
                assert torch.equal(src, ref), (k, name, si, fill, tile, two, "in place")
    finally:
        gpu.tune("ntt_tile", 0)
        gpu.tune("ntt_two_pass", 1)


@pytest.mark.parametrize("which", ["m3+1", "n"])
@pytest.mark.parametrize("si", range(len(SHIFTS)))
@pytest.mark.parametrize("k", SIZES)
def test_in_len_beyond_a_third_runs_the_full_transform(gpu, k, si, which):
    """in_len > m3 is no statement the first pass can use: the result is the transform of the WHOLE vector, element m3 included (a
    short path taken by mistake would drop it).  Tails are clean here: what lies beyond in_len is read."""
    S, shift = _size(gpu, k), SHIFTS[si]
    n, B = S.n, S.batch
    in_len = S.m3 + 1 if which == "m3+1" else n
    try:
        ref = _reference(gpu, S, in_len, shift)          # padded() asserts element in_len - 1 (m3, or n - 1) non-zero
        src = S.padded(in_len, 0)
        assert bool((src[:, S.m3] != 0).any(dim=1).all())
        out = S.out.view(B, n, 4)
        for tile, two in _tunes(k):
            gpu.tune("ntt_tile", tile)
            gpu.tune("ntt_two_pass", two)
            out.fill_(SENTINEL)
            torch.cuda.synchronize()
            gpu.ntt_in_len_device(src.data_ptr(), 0, out.data_ptr(), 0, n, B, in_len, shift)
            assert torch.equal(out, ref), (k, which, si, tile, two)
        # and the short result differs: dropping element m3 is visible in this comparison
        src2 = S.padded(S.m3, 0)
        gpu.ntt_in_len_device(src2.data_ptr(), 0, out.data_ptr(), 0, n, B, S.m3, shift)
        assert not torch.equal(out, ref)
    finally:
        gpu.tune("ntt_tile", 0)
        gpu.tune("ntt_two_pass", 1)


@pytest.mark.parametrize("k", [k for k in SIZES if k > ORACLE_MAX_K])
def test_the_full_path_is_the_oracles_where_it_is_the_only_reference(gpu, k):
    """m3 = 2^19 and 2^21: the cases above compare with the library's full path alone.  One whole random vector per size through that
    path against the oracle (tests/test_gpu_ntt_large.py holds the neighbours 3 * 2^20 and 3 * 2^22)."""
    S = _size(gpu, k)
    src = S.padded(S.n, 0, 1)
    ref = S.ref.view(S.batch, S.n, 4)[:1]
    gpu.ntt_in_len_device(src.data_ptr(), 0, ref.data_ptr(), 0, S.n, 1, 0)
    h = np.ascontiguousarray(S.xv[0].cpu().numpy().view(np.uint64))
    assert np.array_equal(ref[0].cpu().numpy().view(np.uint64), oc.ntt(h, threads=16))


@pytest.mark.parametrize("si", [0, 2])
@pytest.mark.parametrize("k,batch", [(12, 1), (12, 3), (12, 10), (14, 1), (14, 3), (14, 10), (19, 3)])
def test_batches_strides_and_sentinels(gpu, k, batch, si):
    """Batch 1, 3 and 10 (a lane's slots) of DIFFERENT vectors: contiguous, and strided with in_stride != out_stride, both above n,
    sentinel words between the vectors -- out of place and in place (equal strides), with clean and poisoned tails.  The sentinels
    and the input are unchanged afterwards; an in_len or a stride applied to the wrong vector of the batch shows."""
    S, shift = _size(gpu, k, batch), SHIFTS[si]
    n, m3 = S.n, S.m3
    in_stride, out_stride = n + 5, n + 11
    wide_in = torch.empty((batch, in_stride, 4), dtype=torch.int64, device="cuda")
    wide_out = torch.empty((batch, out_stride, 4), dtype=torch.int64, device="cuda")
    for in_len in (m3 // 2 + 8, m3):
        ref = _reference(gpu, S, in_len, shift)
        for fill in (0, POISON):
            src = S.padded(in_len, fill)
            out = S.out.view(batch, n, 4)
            gpu.ntt_in_len_device(src.data_ptr(), 0, out.data_ptr(), 0, n, batch, in_len, shift)
            assert torch.equal(out, ref), (k, batch, in_len, fill, "contiguous")
            wide_in.fill_(SENTINEL)
            wide_in[:, :n] = src
            wide_out.fill_(SENTINEL)
            keep = wide_in.clone()
            torch.cuda.synchronize()
            gpu.ntt_in_len_device(wide_in.data_ptr(), in_stride, wide_out.data_ptr(), out_stride, n, batch, in_len, shift)
            assert torch.equal(wide_out[:, :n], ref), (k, batch, in_len, fill, "strided")
            assert bool((wide_out[:, n:] == SENTINEL).all()) and torch.equal(wide_in, keep)
            gpu.ntt_in_len_device(wide_in.data_ptr(), in_stride, wide_in.data_ptr(), in_stride, n, batch, in_len, shift)
            assert torch.equal(wide_in[:, :n], ref), (k, batch, in_len, fill, "strided in place")
            assert bool((wide_in[:, n:] == SENTINEL).all())


@pytest.mark.parametrize("si", range(len(SHIFTS)))
def test_in_len_is_ignored_where_no_short_path_exists(gpu, si):
    """2^12 points (no radix-3 stage), 3 * 2^10 (unfused: separate decimation / combination kernels) with any in_len, and 3 * 2^12
    with in_len = 0: the public entry point's bytes, on zero-tailed input."""
    shift = SHIFTS[si]
    batch = 3
    for n, in_lens in ((1 << 12, (0, 100, 1365, 1 << 12)), (3 << 10, (0, 100, 1 << 10, 3 << 10)), (3 << 12, (0,))):
        x = torch.empty((batch, n, 4), dtype=torch.int64, device="cuda")
        a, want = torch.empty_like(x), torch.empty_like(x)
        torch.cuda.synchronize()
        gpu.synth_scalars(x.data_ptr(), batch * n, 77 + n % 5)
        gpu.sync()
        x[:, 100:] = 0                                   # every in_len below is a true statement
        torch.cuda.synchronize()
        gpu.ntt_batch_strided_device(x.data_ptr(), n, want.data_ptr(), n, n, batch, coset_shift=shift, sync=True)
        hx = x.cpu().numpy().view(np.uint64)
        for i in range(batch):
            v = np.ascontiguousarray(hx[i])
            assert np.array_equal(want[i].cpu().numpy().view(np.uint64), oc.ntt(v if shift is None else oc.mul_var(v, shift)))
        for in_len in in_lens:
            a.fill_(SENTINEL)
            torch.cuda.synchronize()
            gpu.ntt_in_len_device(x.data_ptr(), n, a.data_ptr(), n, n, batch, in_len, shift)
            assert torch.equal(a, want), (n, in_len)


def test_refusals_are_the_public_entry_points_and_leave_the_library_usable(gpu):
    from uzkge_amd import UzkgeError, _native as N
    S = _size(gpu, 12)
    n, B, in_len = S.n, S.batch, S.m3
    ref = _reference(gpu, S, in_len, None)
    src = S.padded(in_len, POISON)
    out = S.out.view(B, n, 4)
    d, o = src.data_ptr(), out.data_ptr()
    for args, code in (((d, n - 1, o, n - 1, n, 2), N.UZK_ERR_PARAMETER),            # stride < n
                       ((d, n, d, n + 5, n, 2), N.UZK_ERR_PARAMETER),                # in place, unequal strides
                       ((d, 0, o, 0, n, 65536), N.UZK_ERR_PARAMETER),                # batch > 65535
                       ((d, 0, o, 0, 5 << 12, 1), N.UZK_ERR_FFT),                    # no such domain
                       ((d, 0, o, 0, 3 << 23, 1), N.UZK_ERR_FFT)):                   # beyond UZK_NTT_MAX_LOG2_MIXED
        with pytest.raises(UzkgeError) as e:
            gpu.ntt_in_len_device(*args, in_len)
        with pytest.raises(UzkgeError) as pub:
            gpu.ntt_batch_strided_device(*args)
        assert e.value.code == pub.value.code == code, args
        out.fill_(SENTINEL)
        torch.cuda.synchronize()
        gpu.ntt_in_len_device(d, 0, o, 0, n, B, in_len)
        assert torch.equal(out, ref), args


# ---- the contract at its call sites: derive_cosets (in_len = n) and round 3 (in_len = n + 8) ------------------------------------
_chain, _oracle_runs = {}, {}


def _inputs(n):
    """(ChainInputs, its coset tables by the oracle), once per size.  The reference has no Lagrange SRS below 4096 points: any valid
    points serve as commit bases there (nothing below compares a commitment)."""
    import prover_chain as pch
    from chain_oracle import coset_tables
    from uzkge_amd import poly_commit as pc
    if n not in _chain:
        small = pc.parse_srs_g1_wire(open(os.path.join(GOLDEN, "lagrange-srs-4096.bin"), "rb").read()) if n < 4096 else None
        inp = pch.ChainInputs(n, 300 + n % 97, lagrange_wire=small)
        _chain[n] = (inp, coset_tables(inp))
    return _chain[n]


def _lane(inp, seed):
    """Another proof over inp's circuit: its own witness, public input, blinds and challenges."""
    import prover_chain as pch
    if seed is None:
        return inp
    other = pch.ChainInputs(inp.n, seed, lagrange_wire=inp.lagrange_wire)
    x = copy.copy(inp)
    x.seed = seed
    for f in ("w_evals", "wsel_evals", "pi_evals", "beta", "gamma", "alpha", "zeta", "zeta_omega", "alpha_open", "alpha_open2", "blinds_w",
              "blinds_wsel", "blinds_z", "t_rands", "r_scalars"):
        setattr(x, f, getattr(other, f))
    return x


def _tails_and_coefs(b, pr, lanes, want, slots, what):
    """Every one of a lane's ten slots is zero from n + 3 on; the slots in `slots` (device slot, oracle polynomial) hold the oracle's
    blinded coefficients, the blinds' elements [n, n + 3) among them."""
    n = lanes[0].n
    b.sync()
    for i in range(len(lanes)):
        coefs = pr.download(b.PB_COEFS, i).reshape(10, 6 * n, 4)
        assert not coefs[:, n + 3:].any(), (what, i, "a coefficient slot is not zero beyond n + 3")
        for dev, orc in slots:
            assert np.array_equal(coefs[dev, :n + 3], want[i]["coefs"][orc]), (what, i, dev)
        assert any(coefs[dev, n:n + 3].any() for dev, _ in slots)


def _proof(b, cir, pr, lanes, hide_w, with_wsel, shuffle, tables, what):
    """One proof (a lockstep batch of len(lanes)) through the five rounds on `pr`, with the tail check after rounds 1, 2 and 5 and
    round 3's t against the oracle chain."""
    import prover_chain as pch
    from chain_oracle import oracle_chain
    B, n = len(lanes), lanes[0].n
    want = []
    for x in lanes:                                  # the oracle's run of a (lane, kind of proof) is computed once for the whole file
        key = (n, x.seed, shuffle, tuple(hide_w), with_wsel)
        if key not in _oracle_runs:
            _oracle_runs[key] = oracle_chain(x, shuffle=shuffle, hide_w=hide_w, with_wsel=with_wsel, tables=tables, upto_t=True)
        want.append(_oracle_runs[key])
    cat = lambda f: np.concatenate([np.ascontiguousarray(f(x), dtype=np.uint64).reshape(-1, 4) for x in lanes])
    hiding = list(hide_w) + ([pch.HIDE_WSEL] * 3 if with_wsel else [])
    n_first = len(hiding)
    first = [(i, i) for i in range(5)] + ([(5 + i, 5 + i) for i in range(3)] if with_wsel else []) + [(n_first, 8)]
    pr.round1(cir, cat(lambda x: x.w_evals).reshape(B, 5 * n, 4), cat(lambda x: x.wsel_evals).reshape(B, 3 * n, 4) if with_wsel else None,
              np.arange(8, dtype=np.uint32), cat(lambda x: x.pi_evals[:8]).reshape(B, 8, 4), hiding,
              cat(lambda x: np.concatenate([x.blinds_w, x.blinds_wsel]) if with_wsel else x.blinds_w))
    _tails_and_coefs(b, pr, lanes, want, first, (what, "round 1"))
    pr.round2(cat(lambda x: x.beta), cat(lambda x: x.gamma), cat(lambda x: x.blinds_z))
    _tails_and_coefs(b, pr, lanes, want, first + [(n_first + 1, 9)], (what, "round 2"))
    pr.round3(cat(lambda x: x.alpha), cat(lambda x: x.t_rands))
    b.sync()
    for i in range(B):
        assert np.array_equal(pr.download(b.PB_T, i), want[i]["t"]), (what, i, "t")
    pr.round4(cat(lambda x: x.zeta), shuffle)
    pr.round5(cat(lambda x: x.r_scalars[:len(pch.r_plan(shuffle))]), cat(lambda x: x.alpha_open), cat(lambda x: x.alpha_open2))
    _tails_and_coefs(b, pr, lanes, want, first + [(n_first + 1, 9)], (what, "round 5"))


def _circuits(b, inp):
    import prover_chain as pch
    polys = [inp.table_polys[i] for i in range(pch.N_TABLES)]
    mk = lambda shuffle: b.Circuit(inp.n, inp.lagrange_wire, inp.bases[inp.n:], inp.perm, inp.k, inp.anemoi_g, inp.anemoi_g_inv, inp.edwards_a,
                                   polys, shuffle=shuffle, synthetic=True)
    return mk(True), mk(False)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("n", [1 << 11, 1 << 12])
def test_coefficient_slots_stay_zero_beyond_their_blinds_across_proofs_of_one_prover(gpu, n, lanes):
    """m3 = 4096 and 8192: the smallest proofs on the fused path.  ONE private prover, never re-created: a proof with wire selectors
    and maximal hiding degrees (ten slots), then one without selectors (seven slots in another order: pi and z move to slots 5 and
    6, over what the selectors' polynomials left there) and with hiding degrees 2, then the first again.  A stale blind in
    [n + 2, n + 3) or a stale selector polynomial would change t, which is the oracle chain's for every proof.  lanes = 2: the same
    as a lockstep batch (round 3 then transforms all ten slots of every lane, in use or not)."""
    import prover_chain as pch
    b = gpu
    inp, tables = _inputs(n)
    xs = [_lane(inp, None if i == 0 else 7000 + i) for i in range(lanes)]
    full, plain = _circuits(b, inp)
    pr = b.Prover(n, lanes, shared=False)
    try:
        assert not pr.download(b.PB_COEFS).any()                                   # prover_alloc cleared the block
        _proof(b, full, pr, xs, pch.HIDE_W, True, True, tables, "selectors, hiding 3 3 3 2 2")
        _proof(b, plain, pr, xs, (2, 2, 2, 2, 2), False, False, tables, "no selectors, hiding 2")
        _proof(b, full, pr, xs, pch.HIDE_W, True, True, tables, "selectors again")
    finally:
        pr.destroy(); full.release(); plain.release()


@pytest.mark.parametrize("n", [1 << 11, 1 << 12])
def test_derive_cosets_of_full_length_coefficient_forms(gpu, n):
    """derive_cosets transforms in place with in_len = n on 6n-point slots: coefficient forms of full length n with a non-zero top
    coefficient, every table against the oracle's coset FFT."""
    import prover_chain as pch
    b = gpu
    inp, tables = _inputs(n)
    assert all(inp.table_polys[i, n - 1].any() for i in range(pch.N_TABLES))
    full, plain = _circuits(b, inp)
    try:
        for cir, count in ((full, pch.N_TABLES), (plain, 21)):
            assert cir.n_slots == count
            for i in range(count):
                ptr, ln = cir.table(i, coset=True)
                assert ln == 6 * n and np.array_equal(b.dev_download(ptr, (6 * n, 4)), tables[i]), (count, i)
    finally:
        full.release(); plain.release()
