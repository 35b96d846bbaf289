#!/usr/bin/env python3
"""Timing of the batched Groth16 prover (uzk_g16_prove_batch) at the reference's real shape -- the reveal key of tests/golden
(l = 7, m = 4869, h_query of 8191 points) over the stand-in R1CS of tests/g16_cases.py (8185 constraints, n = 8192) -- at batch 1, 8
and 52 (the reveals of one deck):

  one call    uzk_g16_prove_batch on host assignments, the host clock around the call; one more call with uzk_profile_* on gives the
              split by stage (host_g16_*: wall time of a stage, the stream synchronised between stages while profiling) and the
              device time of the kernels inside (g16_*: sparse products, pointwise, scalar rows; ntt_*: the seven transforms; g2_*
              and host_g2_horner: the G2 MSM)
  sequence    the same work through the entry points the library had before, one after another on host arrays, as a host-side prover
              would issue them: uzk_ntt_fr_batch x 3 (inverse, coset forward, coset inverse), uzk_field_op_device x 3 (a o b, - c,
              / (g^n - 1)), uzk_msm_g1_batch x 3 over a_query || alpha || delta etc. registered as SRS handles, uzk_msm_g2_batch.
              NOT counted in the sequence, in its favour: the sparse products <A_i, z> (precomputed here with Python integers), building
              the scalar rows, and the finish (2 scalar multiplications and 2 additions per proof), which a host prover does with its own
              curve library.  This sequence is the yardstick.

  finish      uzk_g16_prove_batch_finish on the same host assignments: the one call with B's Horner chain, C = s A + r B1 + K, the affine
              maps and the blob encoding as kernels (finish="device").  Its column stands beside the one call's, with the spread
              (min .. max) of both over the repetitions; its profiled call gives finish_device (the wall time of the upload of the
              three G1 sums, g16_chains, g16_combine, g16_encode and the copies back) and the new kernels' device times.

All three alternate in ONE process, warm-up first, the median of `--reps` repetitions.
usage: python tools/g16_shape.py [--reps 7] [--out profiles/g16_shape.txt]"""
import argparse, ctypes, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import g16_cases as gc
import g16_ref as gr
import g2_ref as g2
import oracle_c as oc
from uzkge_amd import backend as b
from uzkge_amd.errors import check

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g16_shape.txt"))
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


BATCHES = (1, 8, 52)
BMAX = max(BATCHES)
n, l, nc, m = gc.REAL
R = gr.R

b.init(0)
key, sy = gr.load_real_key(), gc.real_system()
arrays = gr.key_arrays(key, m, l, nc, sy.matrices())
dk = b.Groth16Key.from_arrays(**arrays)
delta = arrays["delta_g1"]
srs_a = b.Srs.from_host(np.concatenate([arrays["a_query"], arrays["alpha_g1"][None], delta[None]]))
srs_b = b.Srs.from_host(np.concatenate([arrays["b_g1_query"], arrays["beta_g1"][None], delta[None]]))
srs_k = b.Srs.from_host(np.concatenate([arrays["l_query"], arrays["h_query"], delta[None]]))
g2_b = b.G2Bases.from_host(np.concatenate([arrays["b_g2_query"], arrays["beta_g2"][None], arrays["delta_g2"][None]]))

zs = [gc.witness(sy, k) for k in range(BMAX)]
rs = [gc.blinds("real-shape", k) for k in range(BMAX)]
z_w = np.stack([oc.fr_from_ints(z) for z in zs])
r_w, s_w = oc.fr_from_ints([r for r, _ in rs]), oc.fr_from_ints([s for _, s in rs])
# the sequence's inputs that the one call computes itself: the evaluation vectors and (for the rows) nothing else
abc = np.zeros((3, BMAX, n, 4), dtype=np.uint64)
for k, z in enumerate(zs):
    for j, M in enumerate(sy.matrices()):
        v = [gc.dot(row, z) for row in M] + ([z[i] for i in range(l)] if j == 0 else [0] * l) + [0] * (n - nc - l)
        abc[j, k] = oc.fr_from_ints(v)
shift = oc.fr_from_ints([5])[0]
shift_inv = oc.fr_from_ints([pow(5, R - 2, R)])[0]
zh_inv = oc.fr_from_ints([pow(pow(5, n, R) - 1, R - 2, R)])[0]
P = lambda x: x.ctypes.data_as(ctypes.c_void_p)


def field_op(op, x, y):
    out = np.empty_like(x)
    check(b.lib.uzk_field_op_device(1, op, P(x), P(y), P(out), x.size // 4))
    return out


def sequence(batch):
    ev = np.ascontiguousarray(abc[:, :batch]).reshape(3 * batch, n, 4)
    ev = b.ntt_batch(ev, inverse=True)
    ev = b.ntt_batch(ev, coset_shift=shift).reshape(3, batch * n, 4)
    t = field_op(2, field_op(0, ev[0], ev[1]), ev[2])
    t = field_op(0, t, np.ascontiguousarray(np.broadcast_to(zh_inv, t.shape)))
    h = b.ntt_batch(t.reshape(batch, n, 4), inverse=True, coset_shift=shift_inv)
    ones = np.broadcast_to(oc.fr_from_ints([1])[0], (batch, 1, 4))
    row_a = np.concatenate([z_w[:batch], ones, r_w[:batch, None]], axis=1)
    row_b = np.concatenate([z_w[:batch], ones, s_w[:batch, None]], axis=1)
    rsn = oc.fr_from_ints([(-r * s) % R for r, s in rs[:batch]])
    row_k = np.concatenate([z_w[:batch, l:], h[:, :n - 1], rsn[:, None]], axis=1)
    return b.msm_batch(srs_a, row_a), b.msm_batch(srs_b, row_b), b.msm_batch(srs_k, row_k), b.msm_g2_batch(g2_b, row_b), h


STAGES = ("host_g16_h", "host_g16_msm_a", "host_g16_msm_b1", "host_g16_msm_k", "host_g16_msm_g2", "host_g16_finish")
say(f"Groth16 prover at the real shape (l = {l}, m = {m}, {nc} constraints, n = {n}), host assignments, median of {a.reps} alternating "
    f"repetitions; {b.lib.uzk_version().decode()}")
say(f"{'batch':>5} | {'one call ms':>11} {'sequence ms':>11} {'seq/one':>7} | {'finish ms':>9} {'one/finish':>10} {'one min..max':>15} {'finish min..max':>15} | one profiled call: "
    f"stages (wall ms), then kernels inside (device ms) ||| one profiled finish call: stages, then the finish kernels (device ms)")
FIN_STAGES = STAGES[:-1] + ("host_g16_finish_device",)
FIN_KERNELS = ("g2_horner", "g2_affine", "g16_chains", "g16_combine", "g16_encode")
for batch in BATCHES:
    one_call = lambda: dk.prove(z_w[:batch], r_w[:batch], s_w[:batch])
    fin_call = lambda: dk.prove(z_w[:batch], r_w[:batch], s_w[:batch], finish="device")
    proofs = one_call()
    assert np.array_equal(fin_call()[0], proofs)                  # the two finishes give the same proofs
    ja, _, _, jb2, h_seq = sequence(batch)
    # the two paths compute the same A, B and h
    assert np.array_equal(b.g1_to_affine(ja[0]), proofs[0, 0:8]) and np.array_equal(b.g2_to_affine(jb2[0]), proofs[0, 8:24])
    assert np.array_equal(dk.h(z_w[:1])[0], h_seq[0])
    t1, t2, t3 = [], [], []
    for _ in range(a.reps):
        b.sync(); t = time.perf_counter(); one_call(); t1.append((time.perf_counter() - t) * 1e3)
        b.sync(); t = time.perf_counter(); fin_call(); t3.append((time.perf_counter() - t) * 1e3)
        b.sync(); t = time.perf_counter(); sequence(batch); t2.append((time.perf_counter() - t) * 1e3)
    b.profile_reset(); b.profile_enable(True)
    one_call(); b.sync()
    b.profile_enable(False)
    tab = b.profile_table()
    stages = " ".join(f"{k.replace('host_g16_', '')}={tab[k][1]:.3f}" for k in STAGES if k in tab)
    grp = {"spmv": 0.0, "ntt": 0.0, "pointwise": 0.0, "scalar_rows": 0.0, "g2_kernels": 0.0, "g2_host_horner": 0.0, "g1_msm_kernels": 0.0, "g1_host_horner": 0.0}
    for k, (_, ms) in tab.items():
        if k in ("g16_transpose", "g16_spmv_slices", "g16_spmv_rows"): grp["spmv"] += ms
        elif k.startswith("ntt_"): grp["ntt"] += ms
        elif k == "g16_pointwise": grp["pointwise"] += ms
        elif k == "g16_scalar_rows": grp["scalar_rows"] += ms
        elif k.startswith("g2_"): grp["g2_kernels"] += ms
        elif k == "host_g2_horner": grp["g2_host_horner"] += ms
        elif k.startswith("msm_"): grp["g1_msm_kernels"] += ms
        elif k == "host_msm_horner": grp["g1_host_horner"] += ms
    b.profile_reset(); b.profile_enable(True)
    fin_call(); b.sync()
    b.profile_enable(False)
    ftab = b.profile_table()
    fstages = " ".join(f"{k.replace('host_g16_', '')}={ftab[k][1]:.3f}" for k in FIN_STAGES if k in ftab)
    fkern = " ".join(f"{k}={ftab[k][1]:.3f}" for k in FIN_KERNELS if k in ftab)
    m1, m2, m3 = float(np.median(t1)), float(np.median(t2)), float(np.median(t3))
    say(f"{batch:>5} | {m1:11.3f} {m2:11.3f} {m2 / m1:7.2f} | {m3:9.3f} {m1 / m3:10.2f} {f'{min(t1):.2f}..{max(t1):.2f}':>15} {f'{min(t3):.2f}..{max(t3):.2f}':>15} | {stages} || "
        + " ".join(f"{k}={v:.3f}" for k, v in grp.items()) + f" ||| {fstages} || {fkern}")
dk.release(); srs_a.release(); srs_b.release(); srs_k.release(); g2_b.release()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
