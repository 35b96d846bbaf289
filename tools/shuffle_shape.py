#!/usr/bin/env python3
"""Timing of the mask and the remask of a shuffle on Baby Jubjub: for n = 1, 52, 4096 cards per call,
  uzk_remark_key_create        the table build (one launch per key; the generator's half exists from the first key on)
  uzk_remark_batch             without and with trace, the whole call, and one profiled call's kernel time (uzk_profile_*: device
                               events; a remask is ONE kernel either way -- remark, or remark_trace per 4096 cards)
  uzk_cp_mask_prove_batch      the whole call
  uzk_cp_mask_verify_batch     the whole call, and one profiled call's split by kernel
  uzk_cp_reveal_verify_batch   the yardstick: the reveal verifier of the same m in the same run
Host arrays in, results out, the host clock around each call (every call ends synchronised); warm-up calls first, then the median of
`--reps` calls, the kinds alternating.  The inputs are made by the library itself (points k_i G by uzk_ed_mul_batch, the proofs by the
two provers over random draws) and every verdict is checked to be 0 before anything is timed.  Shader clock and power are sampled
(rocm-smi, read only) before the first and after the last case.
usage: python tools/shuffle_shape.py [--reps 7] [--out profiles/shuffle_shape.txt]"""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from uzkge_amd import backend as b
from uzkge_amd import reveal as rv

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shuffle_shape.txt"))
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


def profiled(fn, kernels):
    b.profile_reset(); b.profile_enable(True); fn(); b.sync(); b.profile_enable(False)
    tab = b.profile_table()
    return " ".join(f"{tab.get(k, (0, 0.0))[1]:.3f}" for k in kernels)


SIZES = (1, 52, 4096)
VERIFY_KERNELS = ("cp_mask_diff", "cp_transcript", "cp_check", "cp_verdict")
med = lambda xs: float(np.median(xs))
b.init(0)
rng = np.random.default_rng(2026)
scalars = lambda n: rv.scalars_to_wire([int.from_bytes(rng.bytes(31), "little") for _ in range(n)])       # below 2^248 < L
g_wire = rv.points_to_wire([rv.GENERATOR])[0]
pk = b.ed_mul_batch(g_wire, scalars(1))[0]
say(f"mask and remask on Baby Jubjub, median of {a.reps} calls, host clock around each call, ms; {b.lib.uzk_version().decode()}")
say(f"device: {smi()} (idle)")
b.RemarkKey(pk).release()                                          # warm-up: the code object, the generator's half
tk = []
for _ in range(a.reps):
    t = time.perf_counter(); k = b.RemarkKey(pk); tk.append((time.perf_counter() - t) * 1e3); k.release()
b.profile_reset(); b.profile_enable(True); key = b.RemarkKey(pk); b.sync(); b.profile_enable(False)
say(f"uzk_remark_key_create: {med(tk):.3f} (min {min(tk):.3f}, max {max(tk):.3f}); one profiled call, ms: remark_table {b.profile_table().get('remark_table', (0, 0.0))[1]:.3f}")
say(f"{'n':>5} | {'remask':>8} {'kernel':>8} | {'with trace':>10} {'kernel':>8} | {'mask prove':>10} | {'mask verify':>11} {'us/proof':>9} | {'reveal verify':>13} | one profiled mask verify, ms: "
    + " ".join(VERIFY_KERNELS))
for n in SIZES:
    e1, e2, cards = (b.ed_mul_batch(g_wire, scalars(n)) for _ in range(3))
    digits = rng.integers(0, 8, size=(n, 84), dtype=np.uint8)
    perm = rng.permutation(n).astype(np.uint32)
    rs, omegas = scalars(n), scalars(n)
    m1, m2, mproofs = b.cp_mask_prove_batch(pk, cards, rs, omegas)
    sk = scalars(1)[0]
    reveal, rpk, rproofs = b.cp_reveal_prove_batch(sk, e1, omegas)
    stmts = np.ascontiguousarray(np.concatenate([e1, reveal, np.tile(rpk, (n, 1))], axis=1).reshape(n, 6, 4))
    plain = lambda: key.remark_batch(e1, e2, digits, perm)
    traced = lambda: key.remark_batch(e1, e2, digits, perm, want_trace=True)
    prove = lambda: b.cp_mask_prove_batch(pk, cards, rs, omegas)
    verify = lambda: b.cp_mask_verify_batch(pk, cards, m1, m2, mproofs)
    yard = lambda: b.cp_reveal_verify_batch(stmts, rproofs)
    for _ in range(3):                                            # warm-up: workspaces, code objects
        p = plain(); t = traced(); prove(); v = verify(); y = yard()
    assert not v.any() and not y.any() and np.array_equal(p[0], t[0]) and np.array_equal(p[1], t[1])
    tr, tt, tp, tv, ty = [], [], [], [], []
    for _ in range(a.reps):
        tr.append(timed(plain)); tt.append(timed(traced)); tp.append(timed(prove)); tv.append(timed(verify)); ty.append(timed(yard))
    k_plain, k_trace = profiled(plain, ("remark",)), profiled(traced, ("remark_trace",))
    say(f"{n:>5} | {med(tr):8.3f} {k_plain:>8} | {med(tt):10.3f} {k_trace:>8} | {med(tp):10.3f} | {med(tv):11.3f} {med(tv) / n * 1e3:9.1f} | {med(ty):13.3f} | "
        + profiled(verify, VERIFY_KERNELS))
say(f"device: {smi()} (after the last case)")
key.release()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
