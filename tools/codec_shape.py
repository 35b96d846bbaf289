#!/usr/bin/env python3
"""Timing of the point codec: for n = 1, 52, 4869, 22 801 and 2^20 points per call,
  uzk_g1 / g2 / ed_decompress_batch   the whole call (host bytes in, host points out), and one profiled call's kernel time
  uzk_g1 / g2 / ed_compress_batch     the whole call
  the subgroup checks                 uzk_g2_decompress_batch and uzk_ed_decompress_batch with check_subgroup, up to 22 801 points
then the key-level calls over the reference's groth16_pk.bin (tests/golden: 22 801 G1 and 4 872 G2 encodings, 1 041 488 bytes),
  RevealCircuit.from_compressed       validate = False / True, with one profiled call's split by kernel
  RevealCircuit.from_key_bytes        the path this replaces (Python integers), timed once in the same run
Host arrays in, results out, the host clock around each call (every call ends synchronised); warm-up calls first, then the median of
`--reps` calls.  The encodings are the key's own (G1: all of its G1 sections; G2: b_g2_query) and 52 subgroup points of Baby Jubjub,
repeated up to n; every status is checked to be 0 before anything is timed.  Shader clock and power are sampled (rocm-smi, read only)
before the first and after the last case.
usage: python tools/codec_shape.py [--reps 7] [--out profiles/codec_shape.txt]"""
import argparse, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import codec_ref as cr
import ed_ref as ed
from uzkge_amd import backend as b
from uzkge_amd import codec
from uzkge_amd.reveal_cs import RevealCircuit

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_shape.txt"))
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


def median(fn, warm=2):
    for _ in range(warm):
        fn()
    return float(np.median([timed(fn) for _ in range(a.reps)]))


def profiled(fn, kernels):
    b.profile_reset(); b.profile_enable(True); fn(); b.sync(); b.profile_enable(False)
    tab = b.profile_table()
    return " ".join(f"{k} {tab.get(k, (0, 0.0))[1]:.3f}" for k in kernels)


def tiled(raw, width, n):
    src = np.frombuffer(raw, dtype=np.uint8).reshape(-1, width)
    return np.ascontiguousarray(np.resize(src, (n, width)))


SIZES = (1, 52, 4869, 22801, 1 << 20)
SUB_MAX = 22801
b.init(0)
data = cr.key_bytes()
layout = cr.key_layout(data)
g1_raw = b"".join(b"".join(cr.section_encodings(data, layout, s)) for s in cr.SECTIONS if s not in cr.G2_SECTIONS)
g2_raw = b"".join(cr.section_encodings(data, layout, "b_g2_query"))
ed_raw = b"".join(cr.ed_compress(p) for p in ed.rand_subgroup_points(52, 2026))
say(f"point codec, median of {a.reps} calls, host clock around each call, ms (kernel: device events of one profiled call); {b.lib.uzk_version().decode()}")
say(f"device: {smi()} (idle)")
say(f"{'n':>8} | {'g1 dec':>8} {'kernel':>8} {'g1 enc':>8} | {'g2 dec':>8} {'kernel':>8} {'g2 enc':>8} {'g2 dec+sub':>10} {'sub kernel':>10} | "
    f"{'ed dec':>8} {'kernel':>8} {'ed enc':>8} {'ed dec+sub':>10} {'sub kernel':>10} | us per point: g1 g2 ed decode")
for n in SIZES:
    row = []
    per = []
    for raw, width, dec, enc, name in ((g1_raw, 32, lambda e: codec.g1_decompress(e), codec.g1_compress, "g1"),
                                       (g2_raw, 64, lambda e, s=False: codec.g2_decompress(e, s), codec.g2_compress, "g2"),
                                       (ed_raw, 32, lambda e, s=False: codec.ed_decompress(e, s), codec.ed_compress, "ed")):
        e = tiled(raw, width, n)
        pts, st = dec(e)
        assert not st.any()
        back, st2 = enc(pts)
        assert not st2.any() and np.array_equal(back, e)
        t_dec = median(lambda: dec(e))
        k_dec = profiled(lambda: dec(e), [f"codec_{name}_dec"]).split()[1]
        t_enc = median(lambda: enc(pts))
        row.append(f"{t_dec:8.3f} {k_dec:>8} {t_enc:8.3f}")
        per.append(f"{t_dec / n * 1e3:.3f}")
        if name != "g1":
            if n <= SUB_MAX:
                assert not dec(e, True)[1].any()
                t_sub = median(lambda: dec(e, True), warm=1)
                k_sub = profiled(lambda: dec(e, True), [f"codec_{name}_sub"]).split()[1]
                row[-1] += f" {t_sub:10.3f} {k_sub:>10}"
            else:
                row[-1] += f" {'-':>10} {'-':>10}"
    say(f"{n:>8} | " + " | ".join(row) + " | " + " ".join(per))

say("")
say("the reference's groth16_pk.bin (22 801 G1 + 4 872 G2 encodings, 3 596 infinities among them) into a resident reveal circuit, ms")
KERNELS = ("codec_g1_dec", "codec_g2_dec", "codec_g2_sub")


def load(validate):
    RevealCircuit.from_compressed(data, validate=validate).release()


for validate in (False, True):
    t = median(lambda: load(validate), warm=1)
    say(f"from_compressed(validate={validate!s:5}) {t:10.3f}   one profiled call, kernels: {profiled(lambda: load(validate), KERNELS)}")
t0 = time.perf_counter()
old = RevealCircuit.from_key_bytes(data)
t_old = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
parsed = RevealCircuit.parse_key_bytes(data)
t_parse = (time.perf_counter() - t0) * 1e3
old.release()
say(f"from_key_bytes (Python integers, once) {t_old:10.3f}   of which parse_key_bytes, the decoding alone (a second run): {t_parse:.3f}")
t0 = time.perf_counter()
lay = codec.g16_pk_layout(data)
say(f"uzk_g16_pk_layout (host only) {(time.perf_counter() - t0) * 1e3:10.3f}")
say(f"device: {smi()} (after the last case)")
os.makedirs(os.path.dirname(a.out), exist_ok=True)
open(a.out, "w").write("\n".join(lines) + "\n")
