#!/usr/bin/env python3
"""Generates tests/golden/chaum_pedersen_reveal_golden.json from the reference tree (run where /root/reference exists; the JSON file
is what travels).

DATA ONLY -- the numbers of three cases of the reference's contracts/solidity/test/reveal.js:
  "aggregate keys must success"   four public keys and the two coordinates their sum is expected to have
  "reveal verify must success"    pk, the masked card (e2.x, e2.y, e1.x, e1.y), the reveal card and the 160 proof bytes
  "unmask verify must success"    a masked card, four reveal cards and the expected y of the unmasked card
No source text is copied: the script reads the hexadecimal strings of the calls' arguments and of the expectations and writes the
values."""
import hashlib
import json
import os
import re
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "chaum_pedersen_reveal_golden.json")

_HEX = r'"(0x[0-9a-fA-F]+)"'


def _points(text):
    return [{"x": x.lower(), "y": y.lower()} for x, y in re.findall(r"x:\s*" + _HEX + r",\s*y:\s*" + _HEX, text)]


def _case(js, title):
    body = js[js.index(title):]
    return body[:body.index("\n  it(")] if "\n  it(" in body else body


def extract():
    js = open(os.path.join(REF, "contracts/solidity/test/reveal.js")).read()
    agg = _case(js, "aggregate keys must success")
    keys = _points(agg)
    want = re.findall(r"to\.equal\(" + _HEX + r"\)", agg)
    assert len(keys) == 4 and len(want) == 2
    rev = _case(js, "reveal verify must success")
    rev_points = _points(rev)
    rev_words = [w.lower() for w in re.findall(r"^\s*" + _HEX + r",?\s*$", rev, re.M)]
    assert len(rev_points) == 2 and len(rev_words) == 5 and len(rev_words[4]) == 2 + 320
    unm = _case(js, "unmask verify must success")
    unm_points = _points(unm)
    unm_words = [w.lower() for w in re.findall(r"^\s*" + _HEX + r",?\s*$", unm, re.M)]
    unm_y = re.findall(r"to\.equal\(" + _HEX + r"\)", unm)
    assert len(unm_points) == 4 and len(unm_words) == 4 and len(unm_y) == 1
    out = {
        "source": "zypher-game/uzkge: contracts/solidity/test/reveal.js (aggregate keys / reveal verify / unmask verify must success)",
        "masked_card_order": ["e2.x", "e2.y", "e1.x", "e1.y"],
        "proof_word_order": ["a.x", "a.y", "b.x", "b.y", "r"],
        "aggregate_keys": {"keys": keys, "sum": {"x": want[0].lower(), "y": want[1].lower()}},
        "reveal_verify": {"pk": rev_points[0], "masked": rev_words[:4], "reveal": rev_points[1], "proof": rev_words[4][2:]},
        "unmask_verify": {"masked": unm_words, "reveals": unm_points, "y": unm_y[0].lower()},
    }
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("written", OUT, hashlib.sha256(open(OUT, "rb").read()).hexdigest())


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("the reference tree is not present: the committed JSON file is the artefact")
    extract()
