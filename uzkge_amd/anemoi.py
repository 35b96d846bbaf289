"""Anemoi-Jive over BN254's scalar field over arrays of inputs, with the reference's names (uzkge/src/anemoi: AnemoiJive254).  Every
function is one call of the Anemoi layer of the C ABI (include/uzkge_gpu.h, uzk_anemoi_*): one lane per item, every item of a call
with the same lengths.

Elements are integers below r.  A trace is the reference's AnemoiVLHTrace / AnemoiStreamCipherTrace as a dict of its five fields:
input, before_permutation and after_permutation (P x ([x0, x1], [y0, y1])), intermediate_values_before_constant_additions
(P x (14 x [x0, x1], 14 x [y0, y1])) and output."""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

from . import _native as N
from . import backend as b

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
_MONT = (1 << 256) % R
_MONT_INV = pow(_MONT, -1, R)
_MASK = (1 << 64) - 1


def to_wire(values: Sequence[int]) -> np.ndarray:
    """[n, 4]: Montgomery words"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        if not 0 <= v < R:
            raise ValueError("element %d is not below r" % i)
        m = v * _MONT % R
        out[i] = [(m >> (64 * k)) & _MASK for k in range(4)]
    return out


def from_wire(wire: np.ndarray) -> List[int]:
    w = np.asarray(wire, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(r[k]) << (64 * k) for k in range(4)) * _MONT_INV % R for r in w]


def _inputs(inputs: Sequence[Sequence[int]]):
    n = len(inputs)
    length = len(inputs[0]) if n else 0
    if any(len(row) != length for row in inputs):
        raise ValueError("every item of a call has the same length")
    flat = [v for row in inputs for v in row]
    return to_wire(flat).reshape(n, length, 4), length


def _traces(inputs, outputs, tr) -> List[Dict]:
    out = []
    for i, row in enumerate(inputs):
        vals = from_wire(tr[i])
        perms = len(vals) // N.ANEMOI_TRACE_ELEMS
        before, mid, after = [], [], []
        for p in range(perms):
            v = vals[p * N.ANEMOI_TRACE_ELEMS:(p + 1) * N.ANEMOI_TRACE_ELEMS]
            before.append((v[0:2], v[2:4]))
            mid.append(([v[4 + 4 * r:6 + 4 * r] for r in range(14)], [v[6 + 4 * r:8 + 4 * r] for r in range(14)]))
            after.append((v[60:62], v[62:64]))
        out.append({"input": list(row), "before_permutation": before, "intermediate_values_before_constant_additions": mid,
                    "after_permutation": after, "output": outputs[i]})
    return out


def anemoi_permutation(states: Sequence[Sequence[int]]) -> List[List[int]]:
    """[x0, x1, y0, y1] -> the permuted state, for every state"""
    if any(len(s) != 4 for s in states):
        raise ValueError("a state is x0, x1, y0, y1")
    out = from_wire(b.anemoi_permute_batch(to_wire([v for s in states for v in s]).reshape(len(states), 4, 4)))
    return [out[4 * i:4 * i + 4] for i in range(len(states))]


def eval_variable_length_hash(inputs: Sequence[Sequence[int]]) -> List[int]:
    """one hash per input; the inputs of a call have the same length (0 is legal)"""
    wire, length = _inputs(inputs)
    return from_wire(b.anemoi_hash_batch(wire, length))


def eval_variable_length_hash_with_trace(inputs: Sequence[Sequence[int]]) -> List[Dict]:
    wire, length = _inputs(inputs)
    out, tr = b.anemoi_hash_batch(wire, length, want_trace=True)
    return _traces(inputs, from_wire(out), tr)


def eval_stream_cipher(inputs: Sequence[Sequence[int]], output_len: int) -> List[List[int]]:
    """output_len elements per input"""
    wire, length = _inputs(inputs)
    out = from_wire(b.anemoi_stream_batch(wire, output_len, length))
    return [out[output_len * i:output_len * (i + 1)] for i in range(len(inputs))]


def eval_stream_cipher_with_trace(inputs: Sequence[Sequence[int]], output_len: int) -> List[Dict]:
    wire, length = _inputs(inputs)
    out, tr = b.anemoi_stream_batch(wire, output_len, length, want_trace=True)
    flat = from_wire(out)
    return _traces(inputs, [flat[output_len * i:output_len * (i + 1)] for i in range(len(inputs))], tr)
