#!/usr/bin/env python3
"""Timing of the G2 MSM (uzk_msm_g2_batch_device) next to the G1 batched MSM (uzk_msm_g1_batch_device) at the same n and batch:
n in {2^10, 2^12, 4869, 2^14, 2^15}, batch in {1, 8, 52}, scalars resident on the device (uniform, uzk_synth_scalars), the host
clock around the whole call (both calls return the results, so they end synchronised).  G2 and G1 calls alternate in ONE process,
warm-up calls first, the median of `--reps` repetitions; per case one more G2 call with uzk_profile_* on gives the per-kernel split
(device events; host_g2_horner is a host section).  G2 bases: the b_g2_query column of tests/golden/groth16-reveal-b-queries.bin at
n = 4869 (775 infinities: the reference's own workload), multiples (i + 1) H of one of its points elsewhere; G1 bases: random points
(uzk_synth_points_random).  Shader clock and power are sampled (rocm-smi, read only) before the first case and after the last.
The `finish ms` column is uzk_msm_g2_batch_finish on the same inputs (the window sums combined and mapped to affine on the device, the
affine points copied back), measured in the same alternation, with the spread (min .. max) of both G2 entries; its profiled call adds
the split of the new kernels (chunk_sum, horner, affine).
usage: python tools/g2_msm_shape.py [--reps 7] [--out profiles/g2_msm_shape.txt]"""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import bn254_pairing as bp
import g2_ref as g
from uzkge_amd import backend as b

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g2_msm_shape.txt"))
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def smi():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=20).stdout
    except Exception as e:                                        # the figure is a side note; the timing does not depend on it
        return f"rocm-smi unavailable ({type(e).__name__})"
    keep = [l.split(":", 1)[-1].strip() if l.startswith("GPU[0]") else None for l in out.splitlines() if any(k in l for k in ("sclk", "Power"))]
    return " | ".join(k for k in keep if k) or "rocm-smi printed no sclk / power line"


SIZES = (1 << 10, 1 << 12, 4869, 1 << 14, 1 << 15)
BATCHES = (1, 8, 52)
NMAX, BMAX = max(SIZES), max(BATCHES)

b.init(0)
col = g.load_fixture()[1]
h = next(q for q in col if q is not None)
mult, cur = [], None
for _ in range(NMAX):
    cur = bp.g2_add(cur, h)
    mult.append(cur)
g2_column, g2_mult = b.G2Bases.from_host(g.points_to_wire(col)), b.G2Bases.from_host(g.points_to_wire(mult))
d_pts = b.dev_alloc(NMAX * 64)
b.synth_points_random(d_pts, NMAX, 1)
g1 = b.Srs.from_device(d_pts, NMAX)
d_sc = b.dev_alloc(NMAX * BMAX * 32)
b.synth_scalars(d_sc, NMAX * BMAX, 2)
b.sync()

say(f"G2 MSM next to the G1 batched MSM, device scalars, median of {a.reps} alternating repetitions; {b.lib.uzk_version().decode()}")
say(f"device: {smi()} (idle)")
say(f"{'n':>6} {'batch':>5} | {'G2 ms':>9} {'G1 ms':>9} {'G2/G1':>6} | {'finish ms':>9} {'G2/finish':>9} {'G2 min..max':>14} {'finish min..max':>15} | G2 per kernel, ms (one profiled call) "
    f"||| finish per kernel, ms")
for n in SIZES:
    bases = g2_column if n == 4869 else g2_mult
    for batch in BATCHES:
        run_g2 = lambda: b.msm_g2_batch_device(bases, d_sc, n, batch)
        run_g1 = lambda: b.msm_batch_device(g1, d_sc, n, batch)
        run_fin = lambda: b.g2_msm_finish(bases, d_sc, n, batch)
        for _ in range(2):
            run_g2(); run_g1(); run_fin()                         # warm-up: workspaces, code objects
        t2, t1, t3 = [], [], []
        for _ in range(a.reps):
            b.sync(); t = time.perf_counter(); run_g2(); t2.append((time.perf_counter() - t) * 1e3)
            b.sync(); t = time.perf_counter(); run_fin(); t3.append((time.perf_counter() - t) * 1e3)
            b.sync(); t = time.perf_counter(); run_g1(); t1.append((time.perf_counter() - t) * 1e3)
        b.profile_reset(); b.profile_enable(True)
        run_g2(); b.sync()
        b.profile_enable(False)
        split = " ".join(f"{k.replace('g2_', '')}={ms:.3f}" for k, (cnt, ms) in sorted(b.profile_table().items()) if "g2_" in k)
        b.profile_reset(); b.profile_enable(True)
        run_fin(); b.sync()
        b.profile_enable(False)
        fsplit = " ".join(f"{k.replace('g2_', '')}={ms:.3f}" for k, (cnt, ms) in sorted(b.profile_table().items()) if "g2_" in k)
        m2, m1, m3 = float(np.median(t2)), float(np.median(t1)), float(np.median(t3))
        say(f"{n:>6} {batch:>5} | {m2:9.3f} {m1:9.3f} {m2 / m1:6.2f} | {m3:9.3f} {m2 / m3:9.2f} {f'{min(t2):.2f}..{max(t2):.2f}':>14} {f'{min(t3):.2f}..{max(t3):.2f}':>15} | {split} ||| {fsplit}")
say(f"device: {smi()} (after the last case)")
g2_column.release(); g2_mult.release(); g1.release()
b.dev_free(d_pts); b.dev_free(d_sc)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
