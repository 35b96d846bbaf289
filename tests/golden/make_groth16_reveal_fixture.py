#!/usr/bin/env python3
"""Generates tests/golden/groth16_reveal_golden.json from the reference tree (run where /root/reference exists; the JSON file is what
travels).

DATA ONLY -- the numbers of the reference's own golden reveal case, contracts/solidity/test/reveal.js ("reveal with snark verify must
success"): the six public signals of RevealVerifier.verifyRevealWithSnark (mask_card.e1, reveal_card, pk: x and y each) and the eight
proof words in the contract's order a.x, a.y, b.x.c1, b.x.c0, b.y.c1, b.y.c0, c.x, c.y.  No source text is copied: the script reads the
decimal strings of the two array arguments and writes the values."""
import hashlib
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "groth16_reveal_golden.json")


def extract():
    js = open(os.path.join(REF, "contracts/solidity/test/reveal.js")).read()
    case = js[js.index("reveal with snark verify must success"):]
    call = case[case.index("verifyRevealWithSnark("):]
    arrays = re.findall(r"\[(.*?)\]", call, re.S)[:2]
    signals, words = ([int(v) for v in re.findall(r'"(\d+)"', a)] for a in arrays)
    assert len(signals) == 6 and len(words) == 8
    out = {
        "source": "zypher-game/uzkge: contracts/solidity/test/reveal.js (reveal with snark verify must success)",
        "public_signals": [str(v) for v in signals],
        "proof_words": [str(v) for v in words],
        "proof_word_order": ["a.x", "a.y", "b.x.c1", "b.x.c0", "b.y.c1", "b.y.c0", "c.x", "c.y"],
    }
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("written", OUT, hashlib.sha256(open(OUT, "rb").read()).hexdigest())


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("the reference tree is not present: the committed JSON file is the artefact")
    extract()
