#!/usr/bin/env python3
"""Cuts the two byte ranges of the reference's Groth16 proving key that groth16-reveal-b-queries.bin leaves out (run where the reference
tree exists): with them the whole key is in tests/golden/.
usage: python make_groth16_key_fixture.py <reference>/shuffle/parameters/groth16_pk.bin

`shuffle/parameters/groth16_pk.bin` (ark-serialize, compressed):
  groth16-reveal-head.bin  bytes [0, 156336): alpha_g1 32 B | beta_g2, gamma_g2, delta_g2 64 B each | u64 LE 7 | 7 x 32 B gamma_abc_g1 |
                           beta_g1 32 B | delta_g1 32 B | u64 LE 4869 | 4869 x 32 B a_query
  groth16-reveal-tail.bin  bytes [623776, 1041488): u64 LE 8191 | 8191 x 32 B h_query | u64 LE 4862 | 4862 x 32 B l_query"""
import hashlib
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HEAD_HI, TAIL_LO, TOTAL = 156336, 623776, 1041488


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    data = open(sys.argv[1], "rb").read()
    assert len(data) == TOTAL
    head, tail = data[:HEAD_HI], data[TAIL_LO:]
    assert struct.unpack_from("<Q", head, 224)[0] == 7 and struct.unpack_from("<Q", head, 520)[0] == 4869
    assert struct.unpack_from("<Q", tail, 0)[0] == 8191 and struct.unpack_from("<Q", tail, 8 + 32 * 8191)[0] == 4862
    for name, blob in (("groth16-reveal-head.bin", head), ("groth16-reveal-tail.bin", tail)):
        open(os.path.join(HERE, name), "wb").write(blob)
        print(hashlib.sha256(blob).hexdigest(), name)


if __name__ == "__main__":
    main()
