#!/usr/bin/env python3
"""Generates tests/golden/card_maps_golden.json from the reference tree (run where the reference exists; the JSON file is what
travels).

DATA ONLY -- the 54 hexadecimal strings of the table in shuffle/src/card_maps.rs: the y coordinates the reference's index_to_point
turns into card points (get_point_from_y_unchecked(y, true)).  No source text is copied: the script reads the quoted hexadecimal
strings and writes the values."""
import hashlib
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "card_maps_golden.json")


def extract():
    text = open(os.path.join(REF, "shuffle/src/card_maps.rs")).read()
    ys = [y.lower() for y in re.findall(r'"(0x[0-9a-fA-F]{64})"', text)]
    assert len(ys) == 54 and len(set(ys)) == 54
    out = {
        "source": "zypher-game/uzkge: shuffle/src/card_maps.rs (the y coordinates of the 54 card points)",
        "rule": "x is the larger root of x^2 = (1 - y^2) / (1 - d y^2)",
        "y": ys,
    }
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("written", OUT, hashlib.sha256(open(OUT, "rb").read()).hexdigest())


if __name__ == "__main__":
    extract()
