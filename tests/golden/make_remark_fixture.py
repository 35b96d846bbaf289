#!/usr/bin/env python3
"""Generates tests/golden/remark_tables_golden.json from the reference tree: `make_remark_fixture.py <path of the reference tree>`
(the JSON file is what travels).

DATA ONLY -- twelve numbers of the reference's preprocessed remask tables (uzkge/src/shuffle/babyjubjub.rs:
get_preprocessed_generators_x / _y / _dxy, 84 segments of 4 entries each): x, y and dxy of the entries (0, 0), (0, 3), (1, 0) and
(83, 3), as decimal strings.  No source text is copied: the script reads the decimal literals in order and writes four triples."""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "remark_tables_golden.json")
ENTRIES = [(0, 0), (0, 3), (1, 0), (83, 3)]


def extract(ref):
    src = open(os.path.join(ref, "uzkge/src/shuffle/babyjubjub.rs")).read()
    cols = {}
    for name in ("x", "y", "dxy"):
        body = src[src.index("fn get_preprocessed_generators_%s(" % name):]
        nums = re.findall(r'MontFp!\(\s*"(\d+)"\s*\)', body)[:84 * 4]
        assert len(nums) == 84 * 4
        cols[name] = nums
    out = {
        "source": "zypher-game/uzkge: uzkge/src/shuffle/babyjubjub.rs (get_preprocessed_generators_x / _y / _dxy)",
        "layout": "entry (i, j) = (j + 1) 16^i G for i < 84, j < 4",
        "generators": [{"i": i, "j": j, "x": cols["x"][4 * i + j], "y": cols["y"][4 * i + j], "dxy": cols["dxy"][4 * i + j]} for i, j in ENTRIES],
    }
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("written", OUT, hashlib.sha256(open(OUT, "rb").read()).hexdigest())


if __name__ == "__main__":
    if len(sys.argv) < 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_remark_fixture.py <reference tree>  (where the tree is not present, the committed JSON file is the artefact)")
    extract(sys.argv[1])
