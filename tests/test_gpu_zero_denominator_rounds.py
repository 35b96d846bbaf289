"""A zero permutation denominator in round 2 (prover.rs:194-209, helpers.rs:160-220): the proof it belongs to is refused
(UZK_ERR_PARAMETER, "a permutation denominator is zero" -- the reference's batch_inversion has no value for it), whichever lane of
a lockstep batch it sits in, and the proofs that run beside it in a shared round are the proofs their inputs give alone.

One inversion serves every lane (Montgomery's trick over the lanes' denominator products, z_poly_lanes): a zero lane is skipped on
the way up AND on the way back, and a wrong skip would put another lane's inverse -- hence another lane's whole proof -- off.

gamma is the challenge that arrives after round 1, so it is what the test poisons: den(j, i) = w[j][i] + gamma + beta k[pv div n]
omega^(pv mod n) is linear in it (tests/zero_factor.py says the same of the wire value)."""
import copy
import os
import sys
import threading

import numpy as np
import pytest

import bn254_py as opy
import oracle_c as oc
import zero_factor as zf
from util import affine_of

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

from test_gpu_circuit_rounds import _circuit_of, _round_inputs, _run_rounds      # noqa: E402
from test_gpu_coalesce import _alone, _digest      # noqa: E402

ROW, WIRE = 1234, 2


def poisoned(x, cir_inp, row=ROW, wire=WIRE):
    """A copy of the lane's inputs whose gamma makes the denominator of (wire, row) zero -- and no numerator: the slot does not map
    to itself.  Permutation, k and the domain are the circuit's (cir_inp), witness and beta the lane's."""
    n = x.n
    ints = lambda a: oc.fr_to_ints(np.ascontiguousarray(a).reshape(-1, 4))
    pv = int(cir_inp.perm.reshape(5, n)[wire, row])
    assert pv != wire * n + row and row < n - 1
    omega = ints(cir_inp.group_gen)[0]
    beta, w = ints(x.beta)[0], ints(x.w_evals[wire, row])[0]
    y = copy.copy(x)
    y.gamma = oc.fr_from_ints([zf.zero_denominator_gamma(w, beta, ints(cir_inp.k), omega, pv, n)])[0]
    assert (w + ints(y.gamma)[0] + beta * ints(cir_inp.k[wire])[0] * pow(omega, row, opy.R)) % opy.R != 0
    return y


def _round1(prover, cir, lanes):
    import prover_chain as pch
    n, B = lanes[0].n, len(lanes)
    cat = lambda f: np.concatenate([np.ascontiguousarray(f(x), dtype=np.uint64).reshape(-1, 4) for x in lanes])
    return prover.round1(cir, cat(lambda x: x.w_evals).reshape(B, 5 * n, 4), cat(lambda x: x.wsel_evals).reshape(B, 3 * n, 4), np.arange(8, dtype=np.uint32),
                         cat(lambda x: x.pi_evals[:8]).reshape(B, 8, 4), list(pch.HIDE_W) + [pch.HIDE_WSEL] * 3,
                         cat(lambda x: np.concatenate([x.blinds_w, x.blinds_wsel])))


def test_a_lockstep_batch_names_the_proof_whose_denominator_is_zero(gpu):
    """uzk_prover_create_private(n, 3): the bad lane in the middle, first and last (the two ends of the walk back over the lanes'
    prefix products); round 2 fails and names it.  Afterwards the same prover makes three good proofs, each the proof a prover of
    one makes of it."""
    import prover_chain as pch
    from uzkge_amd import UzkgeError
    from uzkge_amd import _native as N
    b = gpu
    n = 1 << 12
    inp = pch.ChainInputs(n, 731)
    lanes = _round_inputs(inp, 3)
    cir = _circuit_of(b, inp)
    p3 = b.Prover(n, 3, shared=False)
    cat = lambda f, ls: np.concatenate([np.ascontiguousarray(f(x), dtype=np.uint64).reshape(-1, 4) for x in ls])
    try:
        for bad in (1, 0, 2):
            _round1(p3, cir, lanes)
            ls = [poisoned(x, inp) if i == bad else x for i, x in enumerate(lanes)]          # gamma arrives after round 1
            with pytest.raises(UzkgeError) as e:
                p3.round2(cat(lambda x: x.beta, ls), cat(lambda x: x.gamma, ls), cat(lambda x: x.blinds_z, ls))
            assert e.value.code == N.UZK_ERR_PARAMETER, bad
            assert f"proof {bad}:" in str(e.value) and "denominator" in str(e.value), (bad, str(e.value))
        o3 = _run_rounds(b, cir, p3, lanes)
        for i, x in enumerate(lanes):
            want = _alone(b, cir, x)
            got = tuple(tuple(affine_of(j) for j in o3[k][i * per:(i + 1) * per]) for k, per in (("cm1", 8), ("cm_z", 1), ("cm_t", 5), ("cm_q", 2)))
            assert got + (o3["evals"][i * 19:(i + 1) * 19].tobytes(),) == want, i
    finally:
        p3.destroy(); cir.release()


def test_a_zero_denominator_in_a_shared_round_fails_alone(gpu):
    """Three threads, one shared prover each, gathered into one lockstep round: thread 1's gamma is poisoned.  It gets the refusal;
    threads 0 and 2 get exactly the proofs their inputs give alone."""
    import prover_chain as pch
    from uzkge_amd import UzkgeError
    from uzkge_amd import _native as N
    b = gpu
    n = 1 << 12
    inp = pch.ChainInputs(n, 831)
    lanes = _round_inputs(inp, 3)
    lanes[1] = poisoned(lanes[1], inp)
    cir = _circuit_of(b, inp)
    errors, result = [], {}
    start = threading.Barrier(3)

    def worker(t):
        try:
            p = b.Prover(n, 1)
            try:
                start.wait()
                try:
                    result[t] = _digest(_run_rounds(b, cir, p, [lanes[t]]))
                except UzkgeError as e:
                    result[t] = (e.code, str(e))
            finally:
                p.destroy()
        except Exception as e:         # surfaced by the main thread
            errors.append((t, repr(e)))
    try:
        want = {t: _alone(b, cir, lanes[t]) for t in (0, 2)}
        b.coalesce_config(4, 200000, 20000, 1)                    # gather for 0.2 s: the three threads join one round
        ths = [threading.Thread(target=worker, args=(t,)) for t in range(3)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errors, errors
        assert result[1][0] == N.UZK_ERR_PARAMETER and "denominator" in result[1][1], result[1]
        assert result[0] == want[0] and result[2] == want[2]
        assert b.coalesce_stats()["widest"] <= 3
    finally:
        b.coalesce_config(8, 0, 0, 0)
        cir.release()
