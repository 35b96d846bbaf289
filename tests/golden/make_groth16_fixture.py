#!/usr/bin/env python3
"""Cuts tests/golden/groth16-reveal-b-queries.bin out of the reference's Groth16 proving key (run where the reference tree exists).

The key is `shuffle/parameters/groth16_pk.bin` (ark-serialize, compressed): the verifying key, beta_g1, delta_g1, a_query, then
b_g1_query and b_g2_query -- the two columns this fixture holds -- then h_query and l_query.  Bytes [156336, 623776) are
`u64 LE 4869 | 4869 x 32 B | u64 LE 4869 | 4869 x 64 B`, byte for byte as the reference reads them at run time."""
import hashlib
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LO, HI = 156336, 623776
N = 4869


def main():
    src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/shuffle/parameters/groth16_pk.bin"
    data = open(src, "rb").read()[LO:HI]
    assert len(data) == HI - LO == 16 + N * 96
    assert struct.unpack_from("<Q", data, 0)[0] == N and struct.unpack_from("<Q", data, 8 + 32 * N)[0] == N
    out = os.path.join(HERE, "groth16-reveal-b-queries.bin")
    open(out, "wb").write(data)
    print(hashlib.sha256(data).hexdigest(), os.path.basename(out))


if __name__ == "__main__":
    main()
