#!/usr/bin/env python3
"""Timing of the Chaum-Pedersen reveal path on Baby Jubjub: for m = 1, 52, 4096 reveals per call,
  uzk_cp_reveal_verify_batch   the whole call, and one profiled call's split by kernel (uzk_profile_*: device events)
  uzk_cp_reveal_prove_batch    the whole call
  uzk_ed_unmask_batch          52 cards x 4 players (once: it does not depend on m)
  uzk_g16_verify_batch         the OTHER verifier of the same statement, the same m, in the same run: copies of the reference's golden
                               Groth16 reveal proof under the reference's key and distinct random 128-bit weights
Host arrays in, results out, the host clock around each call (every call ends synchronised); warm-up calls first, then the median of
`--reps` calls, the four kinds alternating.  The statements are made by the library itself (e1_i = k_i G by uzk_ed_mul_batch, the
proofs by uzk_cp_reveal_prove_batch over random omegas) and every verdict is checked to be 0 before anything is timed.  Shader clock
and power are sampled (rocm-smi, read only) before the first and after the last case.
usage: python tools/cp_shape.py [--reps 7] [--out profiles/cp_shape.txt]"""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import g16_ref as gr
import g16_verify_ref as vr
from uzkge_amd import backend as b
from uzkge_amd import reveal as rv
from uzkge_amd.poly_commit import Groth16VerifierKey, fr_from_int, g16_proof_blob

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cp_shape.txt"))
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


def timed(fn):
    b.sync(); t = time.perf_counter(); fn(); return (time.perf_counter() - t) * 1e3


SIZES = (1, 52, 4096)
KERNELS = ("cp_transcript", "cp_check", "cp_verdict")
b.init(0)
rng = np.random.default_rng(2026)
scalars = lambda n: rv.scalars_to_wire([int.from_bytes(rng.bytes(31), "little") for _ in range(n)])       # below 2^248 < L
g_wire = rv.points_to_wire([rv.GENERATOR])[0]
key = Groth16VerifierKey.from_key_bytes(open(gr.HEAD, "rb").read()[:vr.VK_BYTES])
signals, proof = vr.golden()
raw = np.frombuffer(g16_proof_blob(*proof), dtype=np.uint8)
pub = np.stack([fr_from_int(v) for v in signals])
# 52 cards x 4 players for the unmask: any subgroup points
cards = b.ed_mul_batch(g_wire, scalars(52))
reveals4 = np.ascontiguousarray(b.ed_mul_batch(g_wire, scalars(4 * 52)).reshape(4, 52, 8))
say(f"Chaum-Pedersen reveals on Baby Jubjub, median of {a.reps} calls, host clock around each call, ms; {b.lib.uzk_version().decode()}")
say(f"device: {smi()} (idle)")
say(f"{'m':>5} | {'cp verify':>9} {'min':>8} {'max':>8} {'us/proof':>9} | {'cp prove':>9} | {'unmask 52x4':>11} | {'g16 verify_batch':>16} | one profiled cp verify, ms: " + " ".join(KERNELS))
for m in SIZES:
    sk = scalars(1)[0]
    e1 = b.ed_mul_batch(g_wire, scalars(m))
    omegas = scalars(m)
    reveal, pk, proofs = b.cp_reveal_prove_batch(sk, e1, omegas)
    stmts = np.ascontiguousarray(np.concatenate([e1, reveal, np.tile(pk, (m, 1))], axis=1).reshape(m, 6, 4))
    g16_proofs = np.ascontiguousarray(np.tile(raw, (m, 1)))
    g16_publics = np.ascontiguousarray(np.tile(pub, (m, 1, 1)))
    weights = np.stack([fr_from_int(int.from_bytes(rng.bytes(16), "little") | 1) for _ in range(m)])
    verify = lambda: b.cp_reveal_verify_batch(stmts, proofs)
    prove = lambda: b.cp_reveal_prove_batch(sk, e1, omegas)
    unmask = lambda: b.ed_unmask_batch(cards, reveals4)
    g16 = lambda: key.key.verify_batch(g16_proofs, g16_publics, weights)
    for _ in range(3):                                            # warm-up: workspaces, code objects
        v = verify(); prove(); unmask(); ok, st = g16()
    assert not v.any() and ok and not st.any()
    tv, tp, tu, tg = [], [], [], []
    for _ in range(a.reps):
        tv.append(timed(verify)); tp.append(timed(prove)); tu.append(timed(unmask)); tg.append(timed(g16))
    b.profile_reset(); b.profile_enable(True); verify(); b.sync(); b.profile_enable(False)
    tab = b.profile_table()
    split = " ".join(f"{tab.get(k, (0, 0.0))[1]:.3f}" for k in KERNELS)
    med = float(np.median(tv))
    say(f"{m:>5} | {med:9.3f} {min(tv):8.3f} {max(tv):8.3f} {med / m * 1e3:9.1f} | {float(np.median(tp)):9.3f} | {float(np.median(tu)):11.3f} | {float(np.median(tg)):16.3f} | {split}")
say(f"device: {smi()} (after the last case)")
key.release()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
