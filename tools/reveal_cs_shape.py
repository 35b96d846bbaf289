#!/usr/bin/env python3
"""What the reveal circuit costs on the device, under the reference's own proving key (tests/golden/groth16-reveal-*.bin), median of
seven, batch 1, 8 and 52 (a deck):

  create          uzk_reveal_circuit_create once: the layout on the host, the resident Groth16 key, the table of 2^i G
                  (the parse of the key file in Python is not in it)
  witness         uzk_reveal_witness_batch: host clock around the call, which ends in a synchronise
  witness + prove uzk_reveal_prove_snark_batch
  host-fed prove  uzk_g16_prove_batch fed THE SAME assignments from host memory, their construction not counted: the lower bound of
                  the path being replaced (arkworks' synthesis per card on the CPU, 4869 elements per card uploaded)
  per kernel      a second pass with the library's event profile on (it slows the host: the end-to-end rows come from the pass without)

python tools/reveal_cs_shape.py > profiles/reveal_cs_shape.txt"""
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np

import ed_ref as ed
import g16_ref as gr
from uzkge_amd import backend as b
from uzkge_amd import poly_commit as pc
from uzkge_amd import reveal as rv
from uzkge_amd.reveal_cs import RevealCircuit

REPS = 7
BATCHES = (1, 8, 52)


def median_ms(fn):
    fn()
    b.sync()
    out = []
    for _ in range(REPS):
        t = time.perf_counter()
        fn()
        b.sync()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    b.init(0)
    data = open(gr.HEAD, "rb").read() + open(gr.g2.FIXTURE, "rb").read() + open(gr.TAIL, "rb").read()
    k = RevealCircuit.parse_key_bytes(data)
    g1s = lambda pts: np.stack([pc.g1_wire(p) for p in pts])
    args = [pc.g1_wire(k["alpha_g1"]), pc.g1_wire(k["beta_g1"]), pc.g1_wire(k["delta_g1"]), pc.g2_wire(k["beta_g2"]), pc.g2_wire(k["delta_g2"]),
            g1s(k["a_query"]), g1s(k["b_g1_query"]), g1s(k["l_query"]), g1s(k["h_query"]), np.stack([pc.g2_wire(p) for p in k["b_g2_query"]])]
    made = []
    row = "%-44s %9.3f   (min %.3f, max %.3f)"
    print("reveal circuit, %d variables, domain %d, median of %d, ms" % (b.reveal_cs_info()["n_vars"], b.reveal_cs_info()["domain"], REPS))
    print(row % (("uzk_reveal_circuit_create",) + median_ms(lambda: made.append(b.RevealCircuit(*args)))))
    for c in made[:-1]:
        c.release()
    cir = made[-1]
    rng = random.Random("reveal-cs-shape")
    sk = rv.scalars_to_wire([rng.randrange(1, ed.L)])[0]
    for m in BATCHES:
        e1 = rv.points_to_wire([ed.mul(rng.randrange(1, ed.L), ed.G) for _ in range(m)])
        r = np.stack([pc.fr_from_int(rng.randrange(pc.FR_MODULUS)) for _ in range(m)])
        s = np.stack([pc.fr_from_int(rng.randrange(pc.FR_MODULUS)) for _ in range(m)])
        d_z = b.dev_alloc(32 * cir.n_vars * m)
        print("batch %d" % m)
        print(row % (("  witness_batch",) + median_ms(lambda: cir.witness_batch(sk, e1, d_z))))
        print(row % (("  witness + prove (prove_snark_batch)",) + median_ms(lambda: cir.prove_snark_batch(sk, e1, r, s))))
        z = b.dev_download(d_z, (m, cir.n_vars, 4))
        print(row % (("  prove_batch, the same z from host memory",) + median_ms(lambda: cir.key.prove(z, r, s))))
        assert np.array_equal(cir.key.prove(z, r, s), cir.prove_snark_batch(sk, e1, r, s)[1])
        b.profile_enable(True)
        for name, fn in (("witness_batch", lambda: cir.witness_batch(sk, e1, d_z)), ("prove_snark_batch", lambda: cir.prove_snark_batch(sk, e1, r, s))):
            fn()
            tables = []
            for _ in range(REPS):
                b.profile_reset()
                fn()
                b.sync()
                tables.append(b.profile_table())
            print("  per kernel, %s (event profile on): launches, ms" % name)
            for kernel in sorted(tables[0], key=lambda q: -tables[0][q][1]):
                ms = statistics.median(t.get(kernel, (0, 0.0))[1] for t in tables)
                if ms >= 0.0005:
                    print("    %-36s %4d %9.3f" % (kernel, tables[0][kernel][0], ms))
        b.profile_enable(False)
        b.dev_free(d_z)
    cir.release()


if __name__ == "__main__":
    main()
