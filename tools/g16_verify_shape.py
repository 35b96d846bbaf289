#!/usr/bin/env python3
"""Timing of the batch Groth16 verifier's fold (uzk_g16_verify_fold) under the reference's reveal key (l = 7): m = 1, 8, 52, 364, 4096
proofs per call (copies of the reference's golden reveal proof under distinct random 128-bit weights -- the work per proof does not
depend on its content), host arrays in, the folded points out, the host clock around the whole call (it ends synchronised).  Warm-up
calls first, then `--reps` calls alternating with the yardstick of tools/g2_msm_shape.py: the G1 batched MSM (uzk_msm_g1_batch_device,
batch 1) over m random points with device scalars, in the same process.  Per m one more fold with uzk_profile_* on gives the split:
the four kernels by device events, the two MSMs as host sections around msm_run (with the profile on the stream is drained in front
of them, so they hold the MSMs alone).  Shader clock and power are sampled (rocm-smi, read only) before the first and after the last
case.
usage: python tools/g16_verify_shape.py [--reps 7] [--out profiles/g16_verify_shape.txt]"""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import g16_ref as gr
import g16_verify_ref as vr
from uzkge_amd import backend as b
from uzkge_amd.poly_commit import Groth16VerifierKey, fr_from_int, g16_proof_blob

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g16_verify_shape.txt"))
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


SIZES = (1, 8, 52, 364, 4096)
KERNELS = ("g16v_decode", "g16v_subgroup", "g16v_reduce", "g16v_amul", "host_g16v_msm_x", "host_g16v_msm_c")
b.init(0)
key = Groth16VerifierKey.from_key_bytes(open(gr.HEAD, "rb").read()[:vr.VK_BYTES])
signals, proof = vr.golden()
raw = np.frombuffer(g16_proof_blob(*proof), dtype=np.uint8)
pub = np.stack([fr_from_int(v) for v in signals])
d_pts = b.dev_alloc(max(SIZES) * 64)
b.synth_points_random(d_pts, max(SIZES), 1)
g1 = b.Srs.from_device(d_pts, max(SIZES))
d_sc = b.dev_alloc(max(SIZES) * 32)
b.synth_scalars(d_sc, max(SIZES), 2)
b.sync()
rng = np.random.default_rng(2025)
say(f"uzk_g16_verify_fold, the reference's reveal key (l = {key.n_inputs}), median of {a.reps} calls alternating with the G1 MSM of m points; {b.lib.uzk_version().decode()}")
say(f"device: {smi()} (idle)")
say(f"{'m':>5} | {'fold ms':>9} {'min':>9} {'max':>9} {'us/proof':>9} | {'G1 MSM ms':>9} | one profiled fold, ms: " + " ".join(k.replace("g16v_", "").replace("host_", "") for k in KERNELS))
for m in SIZES:
    proofs = np.ascontiguousarray(np.tile(raw, (m, 1)))
    publics = np.ascontiguousarray(np.tile(pub, (m, 1, 1)))
    weights = np.stack([fr_from_int(int.from_bytes(rng.bytes(16), "little") | 1) for _ in range(m)])
    fold = lambda: key.key.fold(proofs, publics, weights)
    msm = lambda: b.msm_batch_device(g1, d_sc, m, 1)
    for _ in range(3):
        out = fold(); msm()                                       # warm-up: workspaces, code objects, the MSM's plan
    assert not out[5].any()
    tf, tm = [], []
    for _ in range(a.reps):
        b.sync(); t = time.perf_counter(); fold(); tf.append((time.perf_counter() - t) * 1e3)
        b.sync(); t = time.perf_counter(); msm(); tm.append((time.perf_counter() - t) * 1e3)
    b.profile_reset(); b.profile_enable(True); fold(); b.sync(); b.profile_enable(False)
    tab = b.profile_table()
    split = " ".join(f"{tab.get(k, (0, 0.0))[1]:.3f}" for k in KERNELS)
    med = float(np.median(tf))
    say(f"{m:>5} | {med:9.3f} {min(tf):9.3f} {max(tf):9.3f} {med / m * 1e3:9.1f} | {float(np.median(tm)):9.3f} | {split}")
say(f"device: {smi()} (after the last case)")
key.release(); g1.release()
b.dev_free(d_pts); b.dev_free(d_sc)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
