#!/usr/bin/env python3
"""Timing of the SRS check (uzk_srs_check_curve, uzk_srs_fold_powers, uzk_srs_fold_powers_lagrange) at 2^14, 2^20 and 2^24 random
device points (timing needs no SRS: the work does not depend on what the points are), warm-up first, the device synchronised
inside the clock.  Per size, from uzk_profile_*: the curve kernel, the weights kernel, each of the fold's two MSMs (128-bit
scalars); the whole check_curve + fold_powers on the wall clock; in the same run one full-width uzk_msm_g1_device of that size
(random 254-bit scalars); and the CPU oracle's two MSMs over the same points and weights on the CPUs the process may use.  The
Lagrange form at 2^14 and 2^20, with its share of the G1 transform.
usage: python tools/srs_check_shape.py [--reps 5] [--cpu-max-log 24] [--out profiles/srs_check_shape.txt]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np, torch
import oracle_c as oc
from uzkge_amd import backend as b
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="14,20,24")
ap.add_argument("--lagrange-sizes", default="14,20")
ap.add_argument("--cpu-max-log", type=int, default=24, help="largest size the CPU baseline runs at")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srs_check_shape.txt"))
a = ap.parse_args()
SEED = bytes(range(32))
CPUS = min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "0")) or 1 << 30)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        b.sync(); t = time.perf_counter(); fn(); b.sync()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def stats(ts):
    return f"min {min(ts):9.3f} ms  median {sorted(ts)[len(ts) // 2]:9.3f} ms  max {max(ts):9.3f} ms"


def profiled(fn):
    b.profile_reset(); b.profile_enable(True); fn(); b.sync(); b.profile_enable(False)
    return {name: ms for name, (cnt, ms) in b.profile_table().items()}


b.init(0)
say(f"# reps {a.reps}; CPU baseline on {CPUS} threads; times in ms")
for k in [int(x) for x in a.sizes.split(",") if x]:
    n = 1 << k
    pts = torch.empty((n, 8), dtype=torch.int64, device="cuda"); sc = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    b.synth_points_random(pts.data_ptr(), n, 3000 + k); b.synth_scalars(sc.data_ptr(), n, 4000 + k); b.sync()
    srs = b.Srs.from_device(pts.data_ptr(), n)
    report = srs.check_curve(); srs.fold_powers(SEED); b.msm_device(srs, sc.data_ptr(), n)         # warm-up: workspaces, code
    assert report["first_bad"] is None and report["checked"] == n
    t_curve, t_fold, t_full = timed(srs.check_curve, a.reps), timed(lambda: srs.fold_powers(SEED), a.reps), timed(lambda: b.msm_device(srs, sc.data_ptr(), n), a.reps)
    t_both = timed(lambda: (srs.check_curve(), srs.fold_powers(SEED)), a.reps)
    prof = profiled(lambda: (srs.check_curve(), srs.fold_powers(SEED)))
    say(f"n=2^{k:<2d} check_curve            {stats(t_curve)} | srs_curve kernel {prof.get('srs_curve', float('nan')):.3f}")
    say(f"n=2^{k:<2d} fold_powers            {stats(t_fold)} | srs_weights kernel {prof.get('srs_weights', float('nan')):.3f}  MSM left {prof.get('host_srs_fold_msm_left', float('nan')):.3f}"
        f"  MSM right {prof.get('host_srs_fold_msm_right', float('nan')):.3f} (128-bit scalars, under the profiler)")
    say(f"n=2^{k:<2d} check_curve+fold_powers {stats(t_both)}")
    say(f"n=2^{k:<2d} full-width MSM         {stats(t_full)} | fold / full-width MSM (medians) {sorted(t_fold)[len(t_fold) // 2] / sorted(t_full)[len(t_full) // 2]:.2f}")
    if k <= a.cpu_max_log:
        wire = srs.download()
        w = b.srs_fold_weights_device(SEED, n - 1)                      # the host derivation is tested elsewhere; 2^24 Keccak blocks take it a while
        t = time.perf_counter()
        left = oc.msm_pippenger(wire[:n - 1], w, 0, CPUS); right = oc.msm_pippenger(wire[1:], w, 0, CPUS)
        cpu_ms = (time.perf_counter() - t) * 1e3
        got = srs.fold_powers(SEED)
        assert oc.jac_to_affine_ints(got[0]) == oc.jac_to_affine_ints(left) and oc.jac_to_affine_ints(got[1]) == oc.jac_to_affine_ints(right), "device and CPU folds disagree"
        say(f"n=2^{k:<2d} CPU oracle, two MSMs   {cpu_ms:9.1f} ms on {CPUS} threads (same result) | CPU / device fold {cpu_ms / sorted(t_fold)[len(t_fold) // 2]:.0f}x")
        del wire, w
    srs.release(); del pts, sc
for k in [int(x) for x in a.lagrange_sizes.split(",") if x]:
    n = 1 << k
    pts = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    b.synth_points_random(pts.data_ptr(), n, 5000 + k); b.sync()
    srs = b.Srs.from_device(pts.data_ptr(), n)
    srs.fold_powers_lagrange(SEED, n)
    ts = timed(lambda: srs.fold_powers_lagrange(SEED, n), a.reps)
    prof = profiled(lambda: srs.fold_powers_lagrange(SEED, n))
    ntt_ms = sum(ms for name, ms in prof.items() if name.startswith("g1ntt_"))
    say(f"n=2^{k:<2d} fold_powers_lagrange   {stats(ts)} | G1 transform {ntt_ms:.3f}  MSM left {prof.get('host_srs_fold_msm_left', float('nan')):.3f}"
        f"  MSM right {prof.get('host_srs_fold_msm_right', float('nan')):.3f}")
    srs.release(); del pts
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
