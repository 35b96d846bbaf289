#!/usr/bin/env python3
"""What the shuffle circuit costs on the device, for a deck of 52 cards (n = 16 384), median of seven, batch 1 and 8:

  create         uzk_shuffle_circuit_create (layout on the host, table kernels, four refreshes, commit bases; no window tables)
  set_key        uzk_shuffle_circuit_set_key, next to uzk_circuit_refresh_tables of the same 12 tables from HOST evaluation vectors
  witness        uzk_shuffle_witness_batch: remask with trace, variable values, gather, wire selectors, public inputs
  replaced path  what a caller had to do before, on the entry points that were there: uzk_remark_batch with the trace to the host,
                 a host-side gather (NumPy: the trace's values into the variable vector, then value[wiring] over the restatement's
                 wiring), round 1 from host memory.  The matrix, sums and products are NOT recomputed on the host here (they are
                 taken as given), which favours this side; the gather and the trace handling are HOST time
  proof          five rounds from a device witness over the literal circuit, next to tools/prover_chain.py's stand-in of the same n
                 (seeded challenges and r_poly scalars on both sides: the timing does not depend on them)

python tools/shuffle_cs_shape.py > profiles/shuffle_cs_shape.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np

import prover_chain as pch
import shuffle_cs_ref as cr
import shuffle_ref as sr
from uzkge_amd import backend as b
from uzkge_amd import poly_commit as pc
from uzkge_amd.shuffle_cs import HIDE_W, HIDE_WSEL, ShuffleCircuit

CARDS, REPS = 52, 7
GOLDEN = os.path.join(ROOT, "tests", "golden")


def median_ms(fn):
    fn()
    b.sync()
    out = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        b.sync()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def main():
    b.init(0)
    e = sr.e
    n = b.shuffle_cs_info(CARDS)["n"]
    inp = pch.ChainInputs(n, 7)
    lag, mono = inp.lagrange_wire, inp.mono_wire
    k = np.stack([pc.fr_from_int(v) for v in (1, 2, 3, 4, 5)])
    made = []

    def create():
        made.append(ShuffleCircuit.create(CARDS, lag, mono, k))
    print("shuffle circuit, %d cards, n = %d, median of %d, ms" % (CARDS, n, REPS))
    print("create                               %9.3f" % median_ms(create))
    for c in made[:-1]:
        c.release()
    cir = made[-1]
    pk = e.mul(123456789, sr.G)
    key = b.RemarkKey(e.points_wire([pk])[0])
    print("set_key (12 tables from T_pk)        %9.3f" % median_ms(lambda: cir.set_key(key)))
    _, _, ev = cir.test_tables(key)
    host_evals = np.ascontiguousarray(ev[19:31])
    print("uzk_circuit_refresh_tables, 12 host  %9.3f" % median_ms(lambda: cir.refresh_tables(pch.T_QPK, host_evals, want_polys=False)))
    cs = cr.layout(CARDS)
    wiring = np.array(cs.wiring, dtype=np.int64)
    trace_vars = np.array([v for row in cr.remark_rows(cs) for j in range(1, 85) for v in (cs.wiring[0][row + j], cs.wiring[1][row + j], cs.wiring[2][row + j],
                                                                                          cs.wiring[3][row + j])], dtype=np.int64)
    rng = np.random.default_rng(3)
    hiding = list(HIDE_W) + [HIDE_WSEL] * 3
    for batch in (1, 8):
        pts = e.rand_subgroup_points(2 * CARDS * batch, 5)
        e1 = e.points_wire(pts[0::2]).reshape(batch, CARDS, 8)
        e2 = e.points_wire(pts[1::2]).reshape(batch, CARDS, 8)
        digits = rng.integers(0, 8, size=(batch, CARDS, 84), dtype=np.uint8)
        perms = np.stack([rng.permutation(CARDS).astype(np.uint32) for _ in range(batch)])
        d_w, d_s = b.dev_alloc(32 * 5 * n * batch), b.dev_alloc(32 * 3 * n * batch)
        print("batch %d" % batch)
        print("  witness_batch                      %9.3f" % median_ms(lambda: cir.witness_batch(key, e1, e2, digits, perms, d_w, d_s)))
        pi, _, _ = cir.witness_batch(key, e1, e2, digits, perms, d_w, d_s)
        ext = b.dev_download(d_w, (batch, 5 * n, 4))
        wsel = b.dev_download(d_s, (batch, 3 * n, 4))
        values = np.zeros((batch, cs.num_vars, 4), dtype=np.uint64)
        values[:, wiring.reshape(-1)] = ext                       # every variable's value, taken as given (see the docstring)
        prover = b.Prover(n, batch, shared=False)
        blinds = np.tile(np.concatenate([inp.blinds_w, inp.blinds_wsel])[None], (batch, 1, 1, 1))
        parts = {}

        def old_path():
            t0 = time.perf_counter()
            traces = [key.remark_batch(e1[i], e2[i], digits[i], perms[i], want_trace=True)[2] for i in range(batch)]
            t1 = time.perf_counter()
            host = np.empty((batch, 5 * n, 4), dtype=np.uint64)
            for i in range(batch):
                values[i, trace_vars] = traces[i].reshape(-1, 4)
                host[i] = values[i, wiring.reshape(-1)]
            t2 = time.perf_counter()
            prover.round1(cir, host, wsel, cir.pi_rows, pi, hiding, blinds)
            b.sync()
            parts.setdefault("remark", []).append((t1 - t0) * 1e3)
            parts.setdefault("gather", []).append((t2 - t1) * 1e3)
            parts.setdefault("round1", []).append((time.perf_counter() - t2) * 1e3)
        total = median_ms(old_path)
        med = {name: statistics.median(v[1:]) for name, v in parts.items()}
        print("  replaced path, whole               %9.3f" % total)
        print("    uzk_remark_batch, trace to host  %9.3f" % med["remark"])
        print("    host gather (NumPy)              %9.3f   HOST" % med["gather"])
        print("    round 1 from host memory         %9.3f" % med["round1"])

        def new_path():
            cir.witness_batch(key, e1, e2, digits, perms, d_w, d_s)
            prover.round1(cir, d_w, d_s, cir.pi_rows, pi, hiding, blinds, on_device=True)
        print("  witness_batch + round 1 on device  %9.3f" % median_ms(new_path))

        def proof():
            prover.round1(cir, d_w, d_s, cir.pi_rows, pi, hiding, blinds, on_device=True)
            prover.round2(np.tile(inp.beta, (batch, 1)), np.tile(inp.gamma, (batch, 1)), np.tile(inp.blinds_z, (batch, 1)))
            prover.round3(np.tile(inp.alpha, (batch, 1)), np.tile(inp.t_rands, (batch, 1)))
            prover.round4(np.tile(inp.zeta, (batch, 1)), True)
            prover.round5(np.tile(inp.r_scalars, (batch, 1)), np.tile(inp.alpha_open, (batch, 1)), np.tile(inp.alpha_open2, (batch, 1)))
        print("  five rounds from the device witness%9.3f   (%d proofs in lockstep)" % (median_ms(proof), batch))
        prover.destroy()
        b.dev_free(d_w)
        b.dev_free(d_s)
    chain = pch.ProverChain(n=n, precompute=False)
    print("tools/prover_chain.py stand-in, one proof, same n, no window tables %9.3f" % median_ms(chain.run))
    chain.release()
    key.release()
    cir.release()


if __name__ == "__main__":
    main()
