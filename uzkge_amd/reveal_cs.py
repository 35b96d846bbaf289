"""The reveal circuit and its witness on the device: a Groth16 reveal proof (shuffle/src/reveal_with_snark.rs; sdk.rs
reveal_card_with_snark; RevealVerifier.sol) from a secret and masked cards, with no host-side constraint synthesis and no upload of
assignments (include/uzkge_gpu.h, "the reveal circuit").

    circuit = RevealCircuit.from_key_bytes(open("groth16_pk.bin", "rb").read())    # once: the key's points, the circuit's own matrices
    w = circuit.witness(sk, cards)                                                 # assignments stay on the device
    statements, proofs = circuit.prove(sk, cards, r, s)                            # 256-byte blobs for Groth16VerifierKey.verify_batch

As everywhere in this library the randomness is the caller's: r and s are one pair of fresh uniform integers below r_mod per card.
Points of the curve are affine integer pairs; a card is (e1, e2) or just e1."""
import struct
from typing import List, Sequence, Tuple

import numpy as np

from . import _native as N
from .errors import UzkgeError
from . import backend as b
from . import poly_commit as pc
from . import reveal as rv


def _e1s(cards) -> List[Tuple[int, int]]:
    return [c[0] if isinstance(c[0], (tuple, list)) else tuple(c) for c in cards]


def proof_blobs(proofs: np.ndarray) -> List[bytes]:
    """[m, 32] wire proofs (A 8 words, B 16, C 8; Montgomery) -> the 256-byte blobs of pc.g16_proof_blob"""
    inv = pow(1 << 256, -1, pc.FQ_MODULUS)
    out = []
    for row in np.asarray(proofs, dtype=np.uint64).reshape(-1, 32):
        v = [sum(int(row[4 * k + j]) << (64 * j) for j in range(4)) * inv % pc.FQ_MODULUS for k in range(8)]
        nz = lambda *c: None if not any(c) else c
        a, c = nz(v[0], v[1]), nz(v[6], v[7])
        bb = None if not any(v[2:6]) else ((v[2], v[3]), (v[4], v[5]))
        out.append(pc.g16_proof_blob(a, bb, c))
    return out


class RevealWitness:
    """The device-resident assignments of `m` cards and their statements (integers: e1.x e1.y reveal.x reveal.y pk.x pk.y)."""

    def __init__(self, n_vars, m, d_z, statements_wire):
        self.n_vars, self.m, self.d_z, self.statements_wire = n_vars, m, d_z, statements_wire
        self.statements = [tuple(c for p in rv.points_from_wire(row) for c in p) for row in statements_wire]

    def download(self) -> np.ndarray:
        return b.dev_download(self.d_z, (self.m, self.n_vars, 4))

    def release(self) -> None:
        if self.d_z:
            b.dev_free(self.d_z)
            self.d_z = 0


class RevealCircuit(b.RevealCircuit):
    @staticmethod
    def parse_key_bytes(data: bytes) -> dict:
        """ark-serialize (compressed) ProvingKey<Bn254>: vk = alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | Vec gamma_abc_g1, then beta_g1 |
        delta_g1 | Vec a_query | Vec b_g1_query | Vec b_g2_query | Vec h_query | Vec l_query (a Vec: u64 LE length, then the elements)."""
        pos = [0]

        def take(width, f):
            if pos[0] + width > len(data):
                raise UzkgeError(N.UZK_ERR_PARAMETER, "RevealCircuit: the key ends inside an element")
            pos[0] += width
            return f(data[pos[0] - width:pos[0]])

        g1 = lambda: take(32, pc._g1_decompress)
        g2 = lambda: take(64, pc._g2_decompress)

        def vec(f):
            n = take(8, lambda w: struct.unpack("<Q", w)[0])
            if n > (len(data) - pos[0]) // 32:
                raise UzkgeError(N.UZK_ERR_PARAMETER, "RevealCircuit: a vector of %d elements does not fit the key" % n)
            return [f() for _ in range(n)]

        k = dict(alpha_g1=g1(), beta_g2=g2(), gamma_g2=g2(), delta_g2=g2())
        k["gamma_abc_g1"] = vec(g1)
        k["beta_g1"], k["delta_g1"] = g1(), g1()
        for name, f in (("a_query", g1), ("b_g1_query", g1), ("b_g2_query", g2), ("h_query", g1), ("l_query", g1)):
            k[name] = vec(f)
        if pos[0] != len(data):
            raise UzkgeError(N.UZK_ERR_PARAMETER, "RevealCircuit: %d bytes behind the key" % (len(data) - pos[0]))
        return k

    @classmethod
    def from_key_bytes(cls, data: bytes) -> "RevealCircuit":
        k = cls.parse_key_bytes(data)
        g1s = lambda pts: np.stack([pc.g1_wire(p) for p in pts]) if pts else np.zeros((0, 8), dtype=np.uint64)
        g2s = lambda pts: np.stack([pc.g2_wire(p) for p in pts]) if pts else np.zeros((0, 16), dtype=np.uint64)
        self = cls(pc.g1_wire(k["alpha_g1"]), pc.g1_wire(k["beta_g1"]), pc.g1_wire(k["delta_g1"]), pc.g2_wire(k["beta_g2"]), pc.g2_wire(k["delta_g2"]),
                   g1s(k["a_query"]), g1s(k["b_g1_query"]), g1s(k["l_query"]), g1s(k["h_query"]), g2s(k["b_g2_query"]), n_inputs=len(k["gamma_abc_g1"]))
        self.vk_points = (k["alpha_g1"], k["beta_g2"], k["gamma_g2"], k["delta_g2"], k["gamma_abc_g1"])
        return self

    @classmethod
    def from_compressed(cls, data: bytes, validate: bool = False) -> "RevealCircuit":
        """`from_key_bytes` with every point of the key decoded on the device (uzk_reveal_circuit_create_compressed): one launch for the
        22 801 G1 encodings of the reference's key, one for its 4 872 G2 encodings.  validate: also the subgroup check of the G2
        points; a point that fails any check is refused with its section and index.  vk_points is not filled in: make the verifying
        key with Groth16VerifierKey.from_compressed(data)."""
        import ctypes
        raw = np.frombuffer(bytes(data), dtype=np.uint8)
        h = ctypes.c_uint64(0)
        b.check(b.lib.uzk_reveal_circuit_create_compressed(raw.ctypes.data_as(ctypes.c_void_p) if raw.size else None, raw.size, int(bool(validate)), ctypes.byref(h)))
        self = cls.__new__(cls)
        self.handle = h.value
        k = ctypes.c_uint64(0)
        b.check(b.lib.uzk_reveal_circuit_key(self.handle, ctypes.byref(k)))
        self.key = b.Groth16Key(k.value)
        self.n_vars = self.key.n_vars
        return self

    def witness(self, sk: int, cards) -> RevealWitness:
        e1 = rv.points_to_wire(_e1s(cards))
        m = e1.shape[0]
        d_z = b.dev_alloc(32 * self.n_vars * max(m, 1))
        try:
            st = self.witness_batch(rv.scalars_to_wire([sk])[0], e1, d_z)
        except Exception:
            b.dev_free(d_z)
            raise
        return RevealWitness(self.n_vars, m, d_z, st)

    def prove(self, sk: int, cards, r: Sequence[int], s: Sequence[int], finish: str = "host"):
        """(statements, proofs): per card the six integers e1.x e1.y reveal.x reveal.y pk.x pk.y and the 256-byte proof blob.
        finish="device": the proofs are finished and encoded on the device (uzk_reveal_prove_snark_batch_finish); the same blobs."""
        if finish not in ("host", "device"):
            raise ValueError("finish is 'host' or 'device'")
        e1 = rv.points_to_wire(_e1s(cards))
        if len(r) != e1.shape[0] or len(s) != e1.shape[0]:
            raise ValueError("one pair of blinds per card")
        frs = lambda vals: np.stack([pc.fr_from_int(int(v)) for v in vals]) if len(vals) else np.zeros((0, 4), dtype=np.uint64)
        if finish == "device":
            st, _, blobs = self.prove_snark_batch_finish(rv.scalars_to_wire([sk])[0], e1, frs(r), frs(s))
            return [tuple(c for p in rv.points_from_wire(row) for c in p) for row in st], [bytes(row) for row in blobs]
        st, proofs = self.prove_snark_batch(rv.scalars_to_wire([sk])[0], e1, frs(r), frs(s))
        return [tuple(c for p in rv.points_from_wire(row) for c in p) for row in st], proof_blobs(proofs)
