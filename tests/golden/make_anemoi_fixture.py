#!/usr/bin/env python3
"""Generates tests/golden/anemoi_golden.json from the reference tree given as the argument (the JSON file is what travels).

DATA ONLY -- the numbers the reference's uzkge/src/anemoi/tests.rs records:
  test_anemoi_variable_length_hash   the hash of (1, 2, 3, 4)
  test_eval_stream_cipher            the seven outputs of the stream cipher over (1, 2, 3, 4), compared at lengths 2, 4, 6 and 7
No source text is copied: the script reads the decimal strings of the MontFp! literals and the lengths, and writes the values."""
import hashlib
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else ""
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "anemoi_golden.json")


def _case(rs, name):
    body = rs[rs.index("fn " + name + "("):]
    return body[:body.index("\n}\n")]


def extract():
    rs = open(os.path.join(REF, "uzkge/src/anemoi/tests.rs")).read()
    lit = r'MontFp!\(\s*"(\d+)"\s*\)'
    h = _case(rs, "test_anemoi_variable_length_hash")
    s = _case(rs, "test_eval_stream_cipher")
    inputs = [int(v) for v in re.findall(r"F::from\((\d+)u64\)", h)]
    assert inputs == [int(v) for v in re.findall(r"F::from\((\d+)u64\)", s)] == [1, 2, 3, 4]
    hashes = re.findall(lit, h)
    stream = re.findall(lit, s)
    lens = [int(v) for v in re.findall(r"eval_stream_cipher\(&input, (\d+)\)", s)]
    assert len(hashes) == 1 and len(stream) == 7 and lens == [2, 4, 6, 7]
    out = {
        "source": "zypher-game/uzkge: uzkge/src/anemoi/tests.rs (test_anemoi_variable_length_hash, test_eval_stream_cipher)",
        "input": inputs,
        "hash": hashes[0],
        "stream_cipher": {"output": stream, "compared_at_lengths": lens},
    }
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("written", OUT, hashlib.sha256(open(OUT, "rb").read()).hexdigest())


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("usage: make_anemoi_fixture.py <reference tree>   (without one, the committed JSON file is the artefact)")
    extract()
