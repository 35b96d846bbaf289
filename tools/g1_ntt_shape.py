#!/usr/bin/env python3
"""Timing of the G1 transform (uzk_ntt_g1_device): forward and inverse at 2^12, 2^14, 2^16, 2^18 and the bound, random device
points, warm-up first, the device synchronised inside the clock.  Per size: group operations counted from the plan, achieved
operations per second, per-stage time through uzk_profile_*.  At 2^12 also the only route to the same result without the
transform: the batched MSM over the rows of the DFT matrix (uzk_msm_g1_batch_device, rows in chunks of 64, the rows prepared
outside the clock), alternating with the transform, five repetitions each -- the transform must be the faster one.
usage: python tools/g1_ntt_shape.py [--reps 5] [--out profiles/g1_ntt_shape.txt]"""
import argparse, os, re, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from uzkge_amd import backend as b
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g1_ntt_shape.txt"))
a = ap.parse_args()
bound = int(re.search(r"#define UZK_NTT_G1_MAX_LOG2 (\d+)", open(os.path.join(ROOT, "include", "uzkge_gpu.h")).read()).group(1))
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


b.init(0)
for k in sorted({12, 14, 16, 18, bound}):
    n = 1 << k
    src = torch.empty((n, 8), dtype=torch.int64, device="cuda"); dst = torch.empty_like(src)
    torch.cuda.synchronize()
    b.synth_points_random(src.data_ptr(), n, 1000 + k); b.sync()
    for inverse in (False, True):
        fn = lambda: b.ntt_g1_device(src.data_ptr(), dst.data_ptr(), n, inverse=inverse)
        fn(); b.sync()                                        # warm-up: plan, workspace, code
        ts = timed(fn, a.reps)
        dbl, add = b.ntt_g1_plan_info(n, inverse)
        b.profile_reset(); b.profile_enable(True); fn(); b.sync(); b.profile_enable(False)
        tab = b.profile_table()
        stages = " ".join(f"{ms:.3f}" for name, (cnt, ms) in sorted(tab.items()) if name.startswith("g1ntt_stage_"))
        rest = " ".join(f"{name[6:]}={ms:.3f}" for name, (cnt, ms) in sorted(tab.items()) if name.startswith("g1ntt_") and "stage" not in name)
        best = min(ts)
        say(f"n=2^{k:<2d} {'inverse' if inverse else 'forward'}  min {best:9.3f} ms  median {sorted(ts)[len(ts) // 2]:9.3f} ms  max {max(ts):9.3f} ms | "
            f"{dbl} doublings + {add} additions = {(dbl + add) / (best * 1e-3):.3e} group ops/s | stages ms: {stages} | {rest}")
    if k == 12:
        # the route without the transform: out[r] = msm(P, row r of the DFT matrix); rows = the Fr transform of the unit vectors
        rows = torch.zeros((n, n, 4), dtype=torch.int64, device="cuda")
        one = torch.from_numpy(b.field_elementwise("fr", 7, np.array([[1, 0, 0, 0]], dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)).view(np.int64)).cuda()
        rows[torch.arange(n), torch.arange(n)] = one.reshape(4)
        torch.cuda.synchronize()
        for lo in range(0, n, 256):
            b.ntt_batch_device(rows.data_ptr() + lo * n * 32, rows.data_ptr() + lo * n * 32, n, 256, sync=True)
        srs = b.Srs.from_device(src.data_ptr(), n)

        def msm_route():
            for lo in range(0, n, 64):
                b.msm_batch_device(srs, rows.data_ptr() + lo * n * 32, n, 64)
        new = lambda: b.ntt_g1_device(src.data_ptr(), dst.data_ptr(), n)
        msm_route(); new(); b.sync()
        t_new, t_msm = [], []
        for _ in range(5):
            t_new += timed(new, 1); t_msm += timed(msm_route, 1)
        say(f"n=2^12 forward, alternating x5: transform {' '.join(f'{t:.3f}' for t in t_new)} ms | batched MSM over the DFT rows {' '.join(f'{t:.1f}' for t in t_msm)} ms"
            f" | ratio of the medians {sorted(t_msm)[2] / sorted(t_new)[2]:.0f}x")
        # same result?
        got = b.g1_to_affine(b.msm_batch_device(srs, rows.data_ptr() + 5 * n * 32, n, 1)[0])
        assert np.array_equal(got, dst[5].cpu().numpy().view(np.uint64)), "the two routes disagree"
        assert max(t_new) < min(t_msm), "the transform is not faster than the batched MSM over the DFT rows"
        srs.release(); del rows
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
