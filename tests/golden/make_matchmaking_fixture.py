#!/usr/bin/env python3
"""Generates tests/golden/matchmaking_vk_golden.json from the reference tree (run where /root/reference exists; the JSON file is what
travels).

DATA ONLY -- the numbers of matchmaking/parameters/vk-specific.bin, the verifier key the reference generated for zmatchmaking's circuit
of 50 players: a bincode VerifierParamsSplitSpecific { shrunk_cs: TurboCS<Fr>, verifier_params: PlonkVerifierParams } with u64 lengths,
every ark_serialize field a length-prefixed byte blob, G1 points 32-byte compressed (bit 7 of the last byte: y is the larger root; bit 6:
infinity).  The script walks the file to its last byte and writes the 18 commitments as affine integers, k, the Anemoi generator and
its inverse, cs_size, num_vars, the 102 public-input rows and their Lagrange constants.  README_matchmaking.md has the format."""
import json
import os
import struct
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = "matchmaking/parameters/vk-specific.bin"
P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


class Reader:
    def __init__(self, data):
        self.d, self.at = data, 0

    def u64(self):
        v = struct.unpack_from("<Q", self.d, self.at)[0]
        self.at += 8
        return v

    def take(self, n):
        assert self.at + n <= len(self.d), "the file ends inside a field"
        v = self.d[self.at:self.at + n]
        self.at += n
        return v

    def blob(self):
        return self.take(self.u64())

    def usizes(self):
        return [self.u64() for _ in range(self.u64())]


def fr(b):
    v = int.from_bytes(b, "little")
    assert len(b) == 32 and v < R
    return v


def frs(b):
    """an ark_serialize Vec<F>: u64 count, then the elements"""
    count = struct.unpack_from("<Q", b, 0)[0]
    assert len(b) == 8 + 32 * count
    return [fr(b[8 + 32 * i:40 + 32 * i]) for i in range(count)]


def g1(b):
    """a compressed point as [x, y]; the identity as [0, 0]"""
    assert len(b) == 32
    flags, x = b[31] & 0xc0, int.from_bytes(b[:31] + bytes([b[31] & 0x3f]), "little")
    if flags & 0x40:
        assert x == 0
        return [0, 0]
    assert x < P
    y = pow((x * x * x + 3) % P, (P + 1) // 4, P)
    assert y * y % P == (x * x * x + 3) % P, "x is on no point of the curve"
    if (y > P - y) != bool(flags & 0x80):
        y = P - y
    return [x, y]


def main():
    rd = Reader(open(os.path.join(REF, SOURCE), "rb").read())
    # shrunk_cs: TurboCS<Fr> after shrink_to_verifier_only -- everything empty or zero but the three numbers below
    assert frs(rd.blob()) == []                                          # selectors
    assert all(rd.usizes() == [] for _ in range(5))                      # wiring
    assert fr(rd.blob()) == 0                                            # edwards_a
    assert all(frs(rd.blob()) == [] for _ in range(6))                   # the six shuffle tables
    for _ in range(2):                                                   # the preprocessed round keys: zeroed
        keys = rd.blob()
        assert len(keys) == 14 * 2 * 32 and not any(keys)
    assert fr(rd.blob()) == 0 and fr(rd.blob()) == 0                     # anemoi generator and inverse
    assert rd.usizes() == []                                             # anemoi_constraints_indices
    n_iter, num_vars, size = rd.u64(), rd.u64(), rd.u64()
    assert rd.usizes() == [] and rd.usizes() == [] and rd.usizes() == []  # pi rows, pi variables, boolean rows
    assert frs(rd.blob()) == []                                          # shuffle_remark_constraint_indices
    assert rd.take(1) == b"\x01"                                         # verifier_only
    assert frs(rd.blob()) == []                                          # witness
    # verifier_params: PlonkVerifierParams without the "shuffle" feature
    points = lambda: [g1(rd.blob()) for _ in range(rd.u64())]
    cm_q, cm_s = points(), points()
    cm_qb = g1(rd.blob())
    cm_prk = points()
    g, g_inv = fr(rd.blob()), fr(rd.blob())
    k = frs(rd.blob())
    cs_size = rd.u64()
    pi_rows = rd.usizes()
    lagrange = frs(rd.blob())
    assert rd.at == len(rd.d), "%d bytes left over" % (len(rd.d) - rd.at)
    assert (len(cm_q), len(cm_s), len(cm_prk), len(k)) == (8, 5, 4, 5) and g * g_inv % R == 1
    assert n_iter == 0 and size == cs_size and len(pi_rows) == len(lagrange)
    out = {
        "source": "zypher-game/uzkge: " + SOURCE + " (%d bytes, bincode VerifierParamsSplitSpecific)" % len(rd.d),
        "players": 50, "cs_size": cs_size, "num_vars": num_vars,
        "cm_q": cm_q, "cm_s": cm_s, "cm_qb": cm_qb, "cm_prk": cm_prk,
        "anemoi_generator": g, "anemoi_generator_inv": g_inv, "k": k,
        "pi_rows": pi_rows, "pi_lagrange_constants": lagrange,
    }
    json.dump(out, open(os.path.join(HERE, "matchmaking_vk_golden.json"), "w"))       # Python's json carries big integers exactly
    print("written", {name: (len(v) if hasattr(v, "__len__") else v) for name, v in out.items()})


if __name__ == "__main__":
    main()
