#!/usr/bin/env python3
"""Timing of the batch verifier's fold (uzk_verify_fold) under the reference's 52-card verifier key: m = 1, 16, 256, 1024, 4096 proofs
per call (copies of the golden proof under distinct random 128-bit weights -- the work per proof does not depend on its content), host
arrays in, the two folded points out, the clock around the whole call (it ends synchronised).  Warm-up calls first, then `--reps`
calls; per m also the split of ONE more call with uzk_profile_* on (and the transcript kernel's other form, uzk_tune): the four verifier kernels by device events, the two MSMs as host
sections around msm_run (with the profile on, the stream is drained in front of them, so they hold the MSMs alone).
CPU baseline, G1 WORK ONLY: the C oracle's Pippenger (oracle_c.msm_pippenger, 16 threads) over the same assembled terms -- 61 points
and scalars per proof on the right, 2 on the left -- without any transcript, scalar derivation or decoding, which a CPU verifier would
run as well.  Shader clock and power are sampled (rocm-smi, read only) while the largest batch loops.
usage: python tools/verify_shape.py [--reps 9] [--out profiles/verify_shape.txt]"""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import oracle_c as oc
import plonk_batch_ref as br
import plonk_golden_verifier as gv
from uzkge_amd import backend as b
from uzkge_amd.poly_commit import PlonkVerifierKey, fr_from_int, g1_wire

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_shape.txt"))
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


b.init(0)
vk, proof, pi = gv.load_golden(52)
prefix = br.prefix(52)
key = PlonkVerifierKey(vk, prefix)
raw = np.frombuffer(gv.proof_to_bytes(proof), dtype=np.uint8)
pi_wire = np.stack([fr_from_int(v) for v in pi])
left_terms, right_terms = br.terms(vk, proof, pi, prefix)
rng = np.random.default_rng(2024)
say(f"uzk_verify_fold, 52-card key (cs_size {vk['cs_size']}, {len(pi)} public inputs, {raw.size}-byte proofs); {b.lib.uzk_version().decode()}")
say(f"device: {smi()} (idle)")
for m in (1, 16, 256, 1024, 4096):
    proofs = np.ascontiguousarray(np.tile(raw, (m, 1)))
    pis = np.ascontiguousarray(np.tile(pi_wire, (m, 1, 1)))
    rho = [int.from_bytes(rng.bytes(16), "little") | 1 for _ in range(m)]
    weights = np.stack([fr_from_int(v) for v in rho])
    fold = lambda: key.key.fold(proofs, pis, weights)
    for _ in range(3):
        out = fold()                                              # warm-up: workspaces, code objects, the MSM's plan
    assert not out[2].any()
    ts = []
    for _ in range(a.reps):
        b.sync(); t = time.perf_counter(); fold(); ts.append((time.perf_counter() - t) * 1e3)
    # the other form of the transcript kernel (one proof per lane), same call otherwise
    b.tune("verify_transcript", 1)
    fold(); t1 = []
    for _ in range(a.reps):
        b.sync(); t = time.perf_counter(); fold(); t1.append((time.perf_counter() - t) * 1e3)
    b.profile_reset(); b.profile_enable(True); fold(); b.sync(); b.profile_enable(False)
    per_lane = b.profile_table().get("verify_transcript", (0, 0.0))[1]
    b.tune("verify_transcript", 0)
    b.profile_reset(); b.profile_enable(True); fold(); b.sync(); b.profile_enable(False)
    tab = b.profile_table()
    ms = lambda name: tab.get(name, (0, 0.0))[1]
    split = (f"decode {ms('verify_decode'):.3f} transcript {ms('verify_transcript_lanes'):.3f} (one proof per lane: {per_lane:.3f}, its call min {min(t1):.3f}) scalars {ms('verify_scalars'):.3f} reduction {ms('verify_reduce'):.3f} "
             f"MSM R ({45 + 16 * m} points) {ms('host_verify_msm_r'):.3f} MSM L ({2 * m} points) {ms('host_verify_msm_l'):.3f}")
    # CPU baseline: the G1 work alone, over the terms as a CPU verifier meets them (per proof, nothing shared)
    pts_r = np.stack([g1_wire(base) for base, _ in right_terms] * m)
    pts_l = np.stack([g1_wire(base) for base, _ in left_terms] * m)
    sc_r = np.stack([fr_from_int(s * w % br.R) for w in rho for _, s in right_terms])
    sc_l = np.stack([fr_from_int(s * w % br.R) for w in rho for _, s in left_terms])
    cpu = []
    for _ in range(3):
        t = time.perf_counter()
        r_cpu = oc.msm_pippenger(pts_r, sc_r, 0, 16); l_cpu = oc.msm_pippenger(pts_l, sc_l, 0, 16)
        cpu.append((time.perf_counter() - t) * 1e3)
    assert oc.jac_to_affine_ints(r_cpu) == oc.jac_to_affine_ints(out[1]) and oc.jac_to_affine_ints(l_cpu) == oc.jac_to_affine_ints(out[0]), "the fold and the oracle disagree"
    best = min(ts)
    say(f"m={m:<5d} call min {best:9.3f} ms  median {sorted(ts)[len(ts) // 2]:9.3f} ms  max {max(ts):9.3f} ms = {best / m * 1e3:9.1f} us per proof | "
        f"profiled call, ms: {split} | CPU, G1 work only (oracle Pippenger, 16 threads, {63 * m} terms): min {min(cpu):.3f} ms")
    if m == 4096:
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 3.0:
            fold()
        say(f"device: {smi()} (after 3 s of m = 4096 calls)")
key.release()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
