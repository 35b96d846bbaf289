#!/usr/bin/env python3
"""What the matchmaking circuit costs on the device, for 50 players (n = 8 192), median of seven, batch 1, 8, 64 and 1024:

  create         uzk_match_circuit_create (layout on the host, the table kernel, two refreshes, commit bases; no window tables)
  witness        uzk_match_witness_batch: the hash and the stream cipher with their traces left in HBM, steps, variable values, gather
  replaced path  what a caller had to do before, on the entry points that were there:
                   1. uzk_anemoi_hash_batch and uzk_anemoi_stream_batch with the traces to the host
                   2. the witness in the reference's variable order built on the host: 49 divmods per match on Python integers, the
                      exchanges, then NumPy -- one source index per variable into a pool of the match's elements, value[wiring]
                   3. round 1 from host memory
  round 1        a prover holds at most 64 lanes, so batch 1024 is timed without round 1 on both sides

python tools/match_cs_shape.py > profiles/match_cs_shape.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np

import match_cs_ref as mr
import oracle_c as oc
import prover_chain as pch
from uzkge_amd import backend as b
from uzkge_amd import poly_commit as pc
from uzkge_amd.match_cs import HIDE_W, MatchCircuit

PLAYERS, REPS = 50, 7


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


class HostWitness:
    """The reference-order witness of one match from what the Anemoi entry points return, in NumPy where it can be."""

    def __init__(self, cs):
        d = np.array(cs.defs, dtype=np.int64)
        self.kind, self.a, self.b = d[:, 0], d[:, 1], d[:, 2]
        self.n, self.perms = cs.players, mr.stream_permutations(cs.players)
        self.wiring = np.array(cs.wiring, dtype=np.int64).reshape(-1)
        n, p = self.n, self.perms
        # the pool of a match: inputs | seed random commit | hash trace | stream trace | stream outputs | quotients | the integers 0 .. 63
        self.at_scalar, self.at_hash = n, n + 3
        self.at_stream = self.at_hash + 64
        self.at_out = self.at_stream + 64 * p
        self.at_quot = self.at_out + n - 1
        self.at_const = self.at_quot + 64
        self.small = oc.fr_from_ints(list(range(64)))

    def build(self, inputs, seed, rnd, commit, h_trace, s_out, s_trace):
        n, k, a, bb = self.n, self.kind, self.a, self.b
        outs = oc.fr_to_ints(s_out)
        qr = [divmod(outs[i - 1], i + 1) for i in range(1, n)]
        rem = np.zeros(64, dtype=np.int64)
        rem[1:n] = [r for _, r in qr]
        quot = np.zeros((64, 4), dtype=np.uint64)
        quot[1:n] = oc.fr_from_ints([q for q, _ in qr])
        state = np.zeros((n + 1, 64), dtype=np.int64)
        cur = np.arange(64)
        for i in range(1, n):
            state[i] = cur
            r = rem[i]
            cur[i], cur[r] = cur[r], cur[i]
        state[n] = cur
        pool = np.concatenate([inputs, seed[None], rnd[None], commit[None], h_trace.reshape(-1, 4), s_trace.reshape(-1, 4), s_out, quot, self.small])
        zero, ra = self.at_const, rem[a]
        src = np.select(
            [k == mr.CONST, k == mr.INPUT, k == mr.SEED, k == mr.RANDOM, k == mr.COMMIT, k == mr.HASH_TRACE, k == mr.STREAM_TRACE, k == mr.STREAM_OUT,
             k == mr.QUOT, k == mr.REM, k == mr.BIT, k == mr.BIT_SUM, k == mr.PRODUCT, k == mr.PROD_SUM],
            [zero + a, a, self.at_scalar, self.at_scalar + 1, self.at_scalar + 2, self.at_hash + bb, self.at_stream + 64 * a + bb, self.at_out + a,
             self.at_quot + a, zero + ra, zero + (ra == bb), zero + (ra < bb), np.where(ra == bb, state[a, bb], zero),
             np.where(ra < bb, state[a, ra], zero)],
            default=state[np.minimum(a + 1, n), bb])
        return pool[src][self.wiring]


def main():
    b.init(0)
    n = b.match_cs_info(PLAYERS)["n"]
    inp = pch.ChainInputs(n, 7)
    lag, mono = inp.lagrange_wire, inp.mono_wire
    k = np.stack([pc.fr_from_int(v) for v in (1, 2, 3, 4, 5)])
    made = []

    def create():
        made.append(MatchCircuit.create(PLAYERS, lag, mono, k))
    print("matchmaking circuit, %d players, n = %d, median of %d, ms" % (PLAYERS, n, REPS))
    print("create                               %9.3f" % median_ms(create))
    for c in made[:-1]:
        c.release()
    cir = made[-1]
    host = HostWitness(mr.layout(PLAYERS))
    from util import rand_fr_wire
    for batch in (1, 8, 64, 1024):
        inputs = rand_fr_wire(batch * PLAYERS, 11).reshape(batch, PLAYERS, 4)
        seeds, rnds = rand_fr_wire(batch, 12), rand_fr_wire(batch, 13)
        pairs = np.stack([seeds, rnds], axis=1)
        d_w = b.dev_alloc(32 * 5 * n * batch)
        print("batch %d" % batch)
        print("  witness_batch                      %9.3f" % median_ms(lambda: cir.witness_batch(inputs, seeds, rnds, d_w)))
        pi, _, _ = cir.witness_batch(inputs, seeds, rnds, d_w)
        lanes = batch <= 64
        prover = b.Prover(n, batch, shared=False) if lanes else None
        blinds = np.tile(inp.blinds_w[None], (batch, 1, 1, 1)) if lanes else None
        parts = {}
        checked = []

        def old_path():
            t0 = time.perf_counter()
            commit, h_trace = b.anemoi_hash_batch(seeds[:, None], want_trace=True)
            s_out, s_trace = b.anemoi_stream_batch(pairs, PLAYERS - 1, want_trace=True)
            t1 = time.perf_counter()
            ext = np.empty((batch, 5 * n, 4), dtype=np.uint64)
            for i in range(batch):
                ext[i] = host.build(inputs[i], seeds[i], rnds[i], commit[i], h_trace[i], s_out[i], s_trace[i])
            t2 = time.perf_counter()
            if lanes:
                prover.round1(cir, ext, None, cir.pi_rows, pi, list(HIDE_W), blinds)
                b.sync()
            parts.setdefault("anemoi", []).append((t1 - t0) * 1e3)
            parts.setdefault("host", []).append((t2 - t1) * 1e3)
            parts.setdefault("round1", []).append((time.perf_counter() - t2) * 1e3)
            if not checked:                                        # the host path builds the witness the device built
                assert np.array_equal(ext, b.dev_download(d_w, (batch, 5 * n, 4)))
                checked.append(True)
        total = median_ms(old_path)
        med = {name: statistics.median(v[1:]) for name, v in parts.items()}
        print("  replaced path, whole               %9.3f" % total)
        print("    anemoi hash + stream, traces to host %5.3f" % med["anemoi"])
        print("    host witness (Python + NumPy)    %9.3f   HOST" % med["host"])
        if lanes:
            print("    round 1 from host memory         %9.3f" % med["round1"])

            def new_path():
                cir.witness_batch(inputs, seeds, rnds, d_w)
                prover.round1(cir, d_w, None, cir.pi_rows, pi, list(HIDE_W), blinds, on_device=True)
            print("  witness_batch + round 1 on device  %9.3f" % median_ms(new_path))
            prover.destroy()
        b.dev_free(d_w)
    cir.release()


if __name__ == "__main__":
    main()
