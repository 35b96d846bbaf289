"""The reveal prover that ends on the device (uzk_reveal_prove_snark_batch_finish; RevealCircuit.prove(..., finish="device")) under the
reference's own key: the blobs go straight from the prover into Groth16VerifierKey.verify_batch, with no re-encoding in between, and
equal those of the host finish."""
import random

import pytest

import ed_ref as ed
import g16_ref as gr
import g16_verify_ref as vr
import reveal_cs_ref as rc

pytestmark = pytest.mark.gpu
_rng = random.Random("gpu-reveal-finish")
SK = _rng.randrange(1, ed.L)
POINTS = [ed.G] + [ed.mul(_rng.randrange(1, ed.L), ed.G) for _ in range(2)]


@pytest.fixture(scope="module")
def circuit(gpu):
    from uzkge_amd import reveal_cs
    data = open(gr.HEAD, "rb").read() + open(gr.g2.FIXTURE, "rb").read() + open(gr.TAIL, "rb").read()
    c = reveal_cs.RevealCircuit.from_key_bytes(data)
    yield c
    c.release()


@pytest.fixture(scope="module")
def vk(gpu):
    dk = gpu.Groth16VerifierKey(*vr.key_wire(vr.real_vk()))
    yield dk
    dk.release()


def _verify(dk, blobs, publics, seed):
    w = None if len(blobs) == 1 else vr.weights_wire([random.Random(f"reveal-finish-w-{seed}-{i}").randrange(1, 1 << 128) for i in range(len(blobs))])
    accepted, status = dk.verify_batch(b"".join(blobs), vr.publics_wire(publics, dk.n_inputs), w)
    return accepted, [int(s) for s in status]


@pytest.mark.parametrize("m", [1, 3])
def test_device_finished_proofs_verify_and_equal_the_host_finish(gpu, circuit, vk, m):
    pts = POINTS[:m]
    rng = random.Random(f"reveal-finish-blinds-{m}")
    r, s = [rng.randrange(gr.R) for _ in range(m)], [rng.randrange(gr.R) for _ in range(m)]
    statements, blobs = circuit.prove(SK, pts, r, s, finish="device")
    assert len(blobs) == m and all(isinstance(b, bytes) and len(b) == 256 for b in blobs)
    assert [tuple(st) for st in statements] == [tuple(p) + tuple(ed.mul(SK, p)) + tuple(ed.mul(SK, ed.G)) for p in pts]
    assert _verify(vk, blobs, statements, m) == (True, [0] * m)
    bent = [list(st) for st in statements]
    bent[m - 1][2] = (bent[m - 1][2] + 1) % rc.Q
    assert _verify(vk, blobs, bent, m) == (False, [0] * m)
    host_statements, host_blobs = circuit.prove(SK, pts, r, s, finish="host")
    assert host_statements == statements and host_blobs == blobs


def test_reveal_with_snark_passes_finish_through(gpu, circuit, vk):
    from uzkge_amd import reveal as rv
    cards = [(p, p) for p in POINTS[:2]]
    reveals, blobs, pk = rv.reveal_with_snark(SK, cards, circuit, [5, 6], [7, 8], finish="device")
    assert (reveals, blobs, pk) == rv.reveal_with_snark(SK, cards, circuit, [5, 6], [7, 8])
    statements = [tuple(c[0]) + tuple(rvl) + tuple(pk) for c, rvl in zip(cards, reveals)]
    assert _verify(vk, blobs, statements, "rws") == (True, [0, 0])
