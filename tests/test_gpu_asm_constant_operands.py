"""The assembly field primitives on operands the COMPILER can see.

tests/test_gpu_field_kat.py loads every operand from memory; production code also multiplies by literals (to_mont's R^2,
from_mont's (1, 0, .., 0), a zero Horner start).  A literal word may share a register with any other word the compiler knows
to be equal -- with the zero-initialised carry word of a multi-instruction asm statement too, unless that operand is
early-clobber ("+&v"); the statement's first carry then rewrites the input before a later multiply-add reads it.  Every case
here is a kernel of its own (uzk_test_const_operands: the operation and the two operand forms are template parameters) in
which some words are literals and the rest is loaded.  The expected value of every case is computed in Python integers, never
taken from a device result; the portable device form of the same shape is held to the same value.

Rows per case: 4096 random rows with full 32-bit words (a loaded operand that must be a field element is the row mod M), plus
all pairs of the edge values of test_gpu_field_kat.py, masked to the shape.  A wrong value needs a carry out of a 64-bit
column accumulator, which full random words give in about a quarter of the multi-product statements."""
import functools

import numpy as np
import pytest

import bn254_py as opy
from test_gpu_field_kat import _edge_values
from uzkge_amd.errors import UzkgeError

pytestmark = pytest.mark.gpu

# include/uzkge_gpu_test.h
MUL, MUL_RX, SQR, ADD, SUB, ADD_RX, SUB_RX, DBL, L29_MUL, L29_SQR, L29_MUL2, L29_MULC = range(12)
RT, LO4, W0, R2, E1, ZERO, ONE, MM1, L5, L1, ONE261 = range(11)
OP_NAMES = ["mul", "mul_rx", "sqr", "add", "sub", "add_rx", "sub_rx", "dbl", "l29_mul", "l29_sqr", "l29_mul2", "l29_mulc"]
FORM_NAMES = ["x", "(x0..x3,0,0,0,0)", "(x0,0..0)", "R2", "(1,0..0)", "zero", "one", "M-1", "limbs(l0..l4,0,0,0,0)", "limbs(l0,0..0)",
              "one261"]

_PRODUCT = [(LO4, R2), (R2, LO4), (W0, RT), (RT, W0), (RT, E1), (RT, ZERO), (RT, ONE), (R2, ONE), (MM1, MM1), (LO4, LO4)]
_SUM = [(RT, ZERO), (RT, ONE), (RT, MM1), (ZERO, RT), (ONE, RT), (MM1, RT)]
# the CO_CASES list of uzkge_amd/csrc/fieldops.hip: a triple missing there is refused by the hook (UZK_ERR_PARAMETER)
CASES = {
    MUL: _PRODUCT,
    MUL_RX: _PRODUCT,
    SQR: [(LO4, LO4), (W0, W0), (R2, R2), (MM1, MM1)],
    ADD: _SUM, SUB: _SUM, ADD_RX: _SUM, SUB_RX: _SUM,
    DBL: [(ZERO, ZERO), (ONE, ONE), (MM1, MM1), (LO4, LO4), (W0, W0)],
    L29_MUL: [(L5, RT), (RT, L5), (L1, RT), (RT, L1), (L5, L5), (RT, ONE261), (ONE261, RT), (L1, ONE261)],
    L29_SQR: [(L5, L5), (L1, L1), (ONE261, ONE261)],
    L29_MUL2: [(L5, RT), (RT, L5), (L1, RT), (RT, L1), (RT, ONE261)],
    L29_MULC: [(L5, RT), (L1, RT), (RT, L5), (RT, L1), (RT, ONE261)],
}
N_RANDOM = 4096


def _to_ints(rows):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(rows, dtype="<u8")]


def _to_rows(ints):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), dtype="<u8").reshape(-1, 4).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _raw_operands(mod):
    """(a, b) as Python integers: the random block (every word a full 32-bit word), then the all-pairs edge block."""
    rng = np.random.default_rng(20260 + mod % 1000)
    rand = rng.integers(0, 1 << 63, size=(2, N_RANDOM, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(2, N_RANDOM, 4), dtype=np.uint64)
    e = _edge_values(mod)
    a = np.concatenate([rand[0], np.repeat(e, len(e), axis=0)])
    b = np.concatenate([rand[1], np.tile(e, (len(e), 1))])
    return tuple(_to_ints(a)), tuple(_to_ints(b))


def _shape(form, raw, mod):
    """The operand values a form makes of the raw rows: what the kernel computes with, and so what it is sent."""
    if form == RT:
        return [v % mod for v in raw]             # a loaded field element (the edge values are below M already)
    const = {R2: (1 << 512) % mod, E1: 1, ZERO: 0, ONE: (1 << 256) % mod, MM1: mod - 1, ONE261: (1 << 261) % mod}
    if form in const:
        return [const[form]] * len(raw)
    mask = {LO4: (1 << 128) - 1, W0: (1 << 32) - 1, L5: (1 << 145) - 1, L1: (1 << 29) - 1}[form]
    return [v & mask for v in raw]


def _expected(op, x, y, mod):
    i261 = pow(1 << 261, -1, mod)
    if op in (MUL, MUL_RX):
        return [opy.mont_mul(p, q, mod) for p, q in zip(x, y)]
    if op == SQR:
        return [opy.mont_mul(p, p, mod) for p in x]
    if op in (ADD, ADD_RX):
        return [(p + q) % mod for p, q in zip(x, y)]
    if op in (SUB, SUB_RX):
        return [(p - q) % mod for p, q in zip(x, y)]
    if op == DBL:
        return [2 * p % mod for p in x]
    if op == L29_MUL:
        return [p * q * i261 % mod for p, q in zip(x, y)]
    if op == L29_SQR:
        return [p * p * i261 % mod for p in x]
    if op == L29_MUL2:
        return [(p * q + p * p) * i261 % mod for p, q in zip(x, y)]
    return [p * q % mod for p, q in zip(x, y)]     # mulc: the plain product


@pytest.mark.parametrize("op", list(CASES), ids=lambda o: OP_NAMES[o])
@pytest.mark.parametrize("field,mod", [("fq", opy.P), ("fr", opy.R)], ids=["fq", "fr"])
def test_constant_operand_shapes_match_python_integers(gpu, field, mod, op):
    raw_a, raw_b = _raw_operands(mod)
    wrong = []
    for fa, fb in CASES[op]:
        x, y = _shape(fa, raw_a, mod), _shape(fb, raw_b, mod)
        # literal words of the inputs are ignored by the kernel: send the raw rows there, so that a kernel that did load them shows
        a = _to_rows(x if fa == RT else raw_a)
        b = _to_rows(y if fb == RT else raw_b)
        want = _to_rows(_expected(op, x, y, mod))
        for portable in (False, True):
            got = gpu.const_operands(field, op, fa, fb, a, b, portable=portable)
            bad = int(np.count_nonzero(np.any(got != want, axis=1)))
            if bad:
                first = int(np.flatnonzero(np.any(got != want, axis=1))[0])
                wrong.append("%s %s(%s, %s) %s: %d of %d rows wrong, first row %d (%d of them in the random block)" % (
                    field, OP_NAMES[op], FORM_NAMES[fa], FORM_NAMES[fb], "portable" if portable else "assembly", bad, len(want), first,
                    int(np.count_nonzero(np.any(got[:N_RANDOM] != want[:N_RANDOM], axis=1)))))
    assert not wrong, "\n".join(wrong)


def test_a_triple_without_a_kernel_is_refused(gpu):
    a = np.zeros((1, 4), dtype=np.uint64)
    with pytest.raises(UzkgeError):
        gpu.const_operands("fr", MUL, ONE261, RT, a, a)
