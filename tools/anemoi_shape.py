#!/usr/bin/env python3
"""Timing of Anemoi-Jive on the device: for n = 1, 52, 4096, 65536, 2^20 items per call
  uzk_anemoi_permute_batch     one permutation
  uzk_anemoi_hash_batch        a 1-element hash (one permutation) and a 12-element hash (four: the reveal0 challenge)
  uzk_anemoi_stream_batch      the (2 -> 49) stream cipher of zmatchmaking (17 permutations), without and with its trace
and, in the same run, uzk_cp_reveal_verify0_batch next to uzk_cp_reveal_verify_batch at m = 1, 52, 4096.
Host arrays in, results out, the host clock around each call (every call ends synchronised); two warm-up calls, then the median of
`--reps` calls.  Per-kernel times (uzk_profile_*: device events) come from ONE further call per case, after the timed ones.  Inputs
are random field elements; the first item's result is compared with the first call's before anything is timed (correctness is
tests/test_gpu_anemoi.py's business).  A case whose host arrays would pass --max-host-gib is skipped and says so (the trace of 2^20
stream ciphers is 36 GiB).  Shader clock and power are sampled (rocm-smi, read only) before the first and after the last case.
usage: python tools/anemoi_shape.py [--reps 7] [--out profiles/anemoi_shape.txt]"""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from uzkge_amd import backend as b
from uzkge_amd import reveal as rv

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--max-host-gib", type=float, default=4.0)
ap.add_argument("--sizes", default="1,52,4096,65536,1048576")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anemoi_shape.txt"))
a = ap.parse_args()
lines = []
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


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


def elements(rng, count):
    """count canonical elements as Montgomery words: any words below r are some element's"""
    w = rng.integers(0, 1 << 62, size=(count, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 60) - 1)                           # below 2^252 < r
    return w


def measure(fn, kernel):
    first = fn()
    again = fn()
    same = all(np.array_equal(x, y) for x, y in zip(first, again)) if isinstance(first, tuple) else np.array_equal(first, again)
    assert same, "two calls over the same input differ"
    ts = [timed(fn) for _ in range(a.reps)]
    b.profile_reset(); b.profile_enable(True); fn(); b.sync(); b.profile_enable(False)
    launches, ms = b.profile_table().get(kernel, (0, 0.0))
    return float(np.median(ts)), min(ts), max(ts), launches, ms


b.init(0)
rng = np.random.default_rng(2026)
say(f"Anemoi-Jive (AnemoiJive254) on the device, median of {a.reps} calls, host clock around each call, ms; {b.lib.uzk_version().decode()}")
say(f"device: {smi()} (idle)")
say(f"{'case':<22} {'perms':>5} {'n':>8} | {'median':>9} {'min':>9} {'max':>9} {'us/item':>10} {'ns/perm':>10} | one profiled call: launches, kernel ms")
CASES = (("permute", 4, 0, False, 1), ("hash len 1", 1, 0, False, None), ("hash len 12", 12, 0, False, None), ("stream 2 -> 49", 2, 49, False, None),
         ("stream 2 -> 49 + trace", 2, 49, True, None))
for name, length, out_len, trace, fixed in CASES:
    perms = fixed or b.anemoi_permutations(length, out_len)
    for n in (int(s) for s in a.sizes.split(",")):
        host = n * 32 * (length + max(out_len, 1) + (perms * 64 if trace else 0)) / 2 ** 30
        if host > a.max_host_gib:
            say(f"{name:<22} {perms:>5} {n:>8} | skipped: {host:.1f} GiB of host arrays")
            continue
        x = elements(rng, n * length).reshape(n, length, 4)
        if name == "permute":
            fn, kernel = (lambda x=x: b.anemoi_permute_batch(x)), "anemoi_permute"
        elif out_len == 0:
            fn, kernel = (lambda x=x, length=length: b.anemoi_hash_batch(x, length)), "anemoi_sponge"
        else:
            fn = lambda x=x, length=length, out_len=out_len, trace=trace: b.anemoi_stream_batch(x, out_len, length, want_trace=trace)
            kernel = "anemoi_sponge_trace" if trace else "anemoi_sponge"
        med, lo, hi, launches, ms = measure(fn, kernel)
        say(f"{name:<22} {perms:>5} {n:>8} | {med:9.3f} {lo:9.3f} {hi:9.3f} {med / n * 1e3:10.2f} {med / n / perms * 1e6:10.1f} | {launches} x {kernel}: {ms:.3f}")

say("")
say(f"{'m':>5} | {'cp verify0':>10} {'min':>8} {'max':>8} | {'cp verify':>9} {'min':>8} {'max':>8} | {'cp prove0':>9} {'cp prove':>9} | one profiled verify0, ms: cp_transcript cp_check cp_verdict | verify: cp_transcript")
scalars = lambda n: rv.scalars_to_wire([int.from_bytes(rng.bytes(31), "little") for _ in range(n)])       # below 2^248 < L
g_wire = rv.points_to_wire([rv.GENERATOR])[0]
for m in (1, 52, 4096):
    sk = scalars(1)[0]
    e1 = b.ed_mul_batch(g_wire, scalars(m))
    omegas = scalars(m)
    reveal, pk, proofs0 = b.cp_reveal_prove_batch(sk, e1, omegas, anemoi=True)
    _, _, proofs = b.cp_reveal_prove_batch(sk, e1, omegas)
    stmts = np.ascontiguousarray(np.concatenate([e1, reveal, np.tile(pk, (m, 1))], axis=1).reshape(m, 6, 4))
    verify0 = lambda: b.cp_reveal_verify_batch(stmts, proofs0, anemoi=True)
    verify = lambda: b.cp_reveal_verify_batch(stmts, proofs)
    prove0 = lambda: b.cp_reveal_prove_batch(sk, e1, omegas, anemoi=True)
    prove = lambda: b.cp_reveal_prove_batch(sk, e1, omegas)
    for _ in range(2):
        v0 = verify0(); v = verify(); prove0(); prove()
    assert not v0.any() and not v.any()
    t0, t1, p0, p1 = [], [], [], []
    for _ in range(a.reps):
        t0.append(timed(verify0)); t1.append(timed(verify)); p0.append(timed(prove0)); p1.append(timed(prove))
    b.profile_reset(); b.profile_enable(True); verify0(); b.sync(); b.profile_enable(False)
    tab = b.profile_table()
    split = " ".join(f"{tab.get(k, (0, 0.0))[1]:.3f}" for k in ("cp_transcript", "cp_check", "cp_verdict"))
    b.profile_reset(); b.profile_enable(True); verify(); b.sync(); b.profile_enable(False)
    keccak = b.profile_table().get("cp_transcript", (0, 0.0))[1]
    say(f"{m:>5} | {float(np.median(t0)):10.3f} {min(t0):8.3f} {max(t0):8.3f} | {float(np.median(t1)):9.3f} {min(t1):8.3f} {max(t1):8.3f} | "
        f"{float(np.median(p0)):9.3f} {float(np.median(p1)):9.3f} | {split} | {keccak:.3f}")
say(f"device: {smi()} (after the last case)")
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
