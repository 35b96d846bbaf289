#!/usr/bin/env python3
"""Timing of the pairing product on the device (uzk_pairing_product): n = 1, 2, 55, 367, 4099 pairs (a_i G, (i + 1) H) of known
logarithm (tests/pairing_cases.py), host arrays in, the element of GT out, the host clock around the whole call (it ends
synchronised): the median of `--reps` calls after warm-up.  Per n one more call with uzk_profile_* on gives the split by device
events: the check kernel, the Miller loops, the product tree (all its launches), the final exponentiation.  Then, for m = 52 copies of
the reference's golden reveal proof under its real key, uzk_g16_verify_batch (fold + product, verdict out) next to
uzk_g16_verify_fold (the fold alone, as before this entry point existed) in the same process, alternating.  Shader clock and power are
sampled (rocm-smi, read only) before the first and after the last case.
usage: python tools/pairing_shape.py [--reps 7] [--out profiles/pairing_shape.txt]"""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import g16_ref as gr
import g16_verify_ref as vr
import pairing_cases as pc
from uzkge_amd import backend as b
from uzkge_amd.poly_commit import Groth16VerifierKey, fr_from_int, g16_proof_blob

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_shape.txt"))
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


SIZES = (1, 2, 55, 367, 4099)
KERNELS = ("pairing_check", "pairing_miller", "pairing_prod", "pairing_finalexp")
b.init(0)
p_all, q_all, _ = pc.log_pairs(max(SIZES), "shape")
say(f"uzk_pairing_product, median of {a.reps} calls; {b.lib.uzk_version().decode()}")
say(f"device: {smi()} (idle)")
say(f"{'n':>5} | {'call ms':>9} {'min':>9} {'max':>9} | one profiled call, ms: " + " ".join(k.replace("pairing_", "") for k in KERNELS))
for n in SIZES:
    p, q = p_all[:n], q_all[:n]
    call = lambda: b.pairing_product(p, q)
    for _ in range(3):
        call()
    ts = []
    for _ in range(a.reps):
        b.sync(); t = time.perf_counter(); call(); ts.append((time.perf_counter() - t) * 1e3)
    b.profile_reset(); b.profile_enable(True); call(); b.sync(); b.profile_enable(False)
    tab = b.profile_table()
    split = " ".join(f"{tab.get(k, (0, 0.0))[1]:.3f}" for k in KERNELS)
    say(f"{n:>5} | {float(np.median(ts)):9.3f} {min(ts):9.3f} {max(ts):9.3f} | {split}")

m = 52
key = Groth16VerifierKey.from_key_bytes(open(gr.HEAD, "rb").read()[:vr.VK_BYTES])
signals, proof = vr.golden()
raw = np.frombuffer(g16_proof_blob(*proof), dtype=np.uint8)
pub = np.stack([fr_from_int(v) for v in signals])
rng = np.random.default_rng(2026)
proofs = np.ascontiguousarray(np.tile(raw, (m, 1)))
publics = np.ascontiguousarray(np.tile(pub, (m, 1, 1)))
weights = np.stack([fr_from_int(int.from_bytes(rng.bytes(16), "little") | 1) for _ in range(m)])
verify = lambda: key.key.verify_batch(proofs, publics, weights)
fold = lambda: key.key.fold(proofs, publics, weights)
for _ in range(3):
    ok, st = verify(); fold()
assert ok and not st.any()
tv, tf = [], []
for _ in range(a.reps):
    b.sync(); t = time.perf_counter(); verify(); tv.append((time.perf_counter() - t) * 1e3)
    b.sync(); t = time.perf_counter(); fold(); tf.append((time.perf_counter() - t) * 1e3)
b.profile_reset(); b.profile_enable(True); verify(); b.sync(); b.profile_enable(False)
tab = b.profile_table()
names = ("g16v_decode", "g16v_subgroup", "g16v_reduce", "g16v_amul", "host_g16v_msm_x", "host_g16v_msm_c", "g16v_tail") + KERNELS
say(f"m = {m} reveal proofs (l = {key.n_inputs}), alternating: uzk_g16_verify_batch {float(np.median(tv)):.3f} ms (min {min(tv):.3f}, max {max(tv):.3f}) | "
    f"uzk_g16_verify_fold {float(np.median(tf)):.3f} ms (min {min(tf):.3f}, max {max(tf):.3f})")
say("one profiled uzk_g16_verify_batch, ms: " + " ".join(f"{k.replace('g16v_', '').replace('host_', '').replace('pairing_', '')} {tab.get(k, (0, 0.0))[1]:.3f}" for k in names))
say(f"device: {smi()} (after the last case)")
key.release()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
