"""Fq12 (fq12_29.hpp) and the Miller loop's two steps (pairing.hip) on RAW limbs at the edges of the type they carry across loop
iterations (uzk_test_fq12_raw_kat, uzk_test_miller_step_raw: nothing re-limbed or reduced on the way in, nothing canonicalised on the
way out).  Every component of an operand is a member of q12::El = E2<1, 2>: the representative c or c + M, in normalized or carry-step
limbs, or one of lz29_contract.gen_type's extreme vectors as it is; xP and -yP of a step are members of Lz<Fq29, 1, 4> (c + k M,
k = 0 .. 3).  Every raw output component must lie in El (K = 1, V = 2) AND hold exactly the residue of the reference
(tests/pairing_ref.py, oracle/bn254_pairing.py): a result that is the right residue but 2 M or more, or carries a limb outside K = 1,
canonicalises to the right answer and breaks the next iteration's contract only for some inputs.

The Granger-Scott square, the easy part and the hard part (ops 8 .. 10) are defined on the cyclotomic subgroup only, so their inputs
are residues of pairing_ref.easy_part(x) and only k and the limb shape vary (a digit below 2^6 is rare, so most of their components
have the normalized shape alone); every other operation takes any residue, and there the mixes also draw limb vectors with carry-step
limbs directly (fq12_raw.shaped) and let the residue follow."""
import random
import zlib

import numpy as np
import pytest

import bn254_pairing as bp
import bn254_py as opy
import fq12_raw as fr
import pairing_cases as pc
import pairing_ref as pr

pytestmark = pytest.mark.gpu
P = fr.P
ZERO12 = [(0, 0)] * 6
MODES = ["min", "max"] + ["mix"] * 200


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _fq(rng):
    return int.from_bytes(rng.bytes(40), "little") % P


def _rand_f12(rng):
    return [(_fq(rng), _fq(rng)) for _ in range(6)]


def _reps(rng, a, mode):
    """the element of residues a at every component's smallest representative, its largest, or a random k and shape each"""
    if mode == "min":
        return fr.raw_f12(a, 0)
    if mode == "max":
        return fr.raw_f12(a, 1)
    return fr.raw_f12(a, [int(rng.integers(0, 2)) for _ in range(12)], [bool(rng.integers(0, 2)) for _ in range(12)])


def _elem(rng, mode):
    """(residues, 108 words) of an element with free residues; a mix draws half of its components as shaped limb vectors"""
    if mode != "mix":
        a = _rand_f12(rng)
        return a, _reps(rng, a, mode)
    vs = [fr.shaped(rng) if rng.integers(0, 2) else fr.rep_limbs(_fq(rng), int(rng.integers(0, 2)), True) for _ in range(12)]
    return fr.f12_of_limbs(vs)


def _extreme_elements(rng):
    """(residues, words): gen_type(1, 2, P)'s extreme vectors in all six coefficients at once (each alone, and rotated through the
    components), and in one coefficient -- every coefficient, three pairings of the vectors -- with the rest random"""
    ext = fr.extreme_vectors(rng)
    out = [fr.f12_of_limbs([v] * 12) for v in ext]
    out += [fr.f12_of_limbs([ext[(t + s) % 3] for t in range(12)]) for s in range(3)]
    for i in range(6):
        for s in range(3):
            a, row = _elem(rng, "mix")
            vs = fr.components(row)
            vs[2 * i], vs[2 * i + 1] = ext[s], ext[(s + 1 + i) % 3]
            out.append(fr.f12_of_limbs(vs))
    return out


def _operands(rng, binary):
    """[(a residues, a words, b residues, b words)]: min, max, 200 mixes, the extreme elements, the edge elements at both k"""
    out = []
    for mode in MODES:
        a, ra = _elem(rng, mode)
        b, rb = _elem(rng, mode)
        out.append((a, ra, b, rb))
    ext = _extreme_elements(rng)
    for i, (a, ra) in enumerate(ext):
        b, rb = ext[(i + 1) % 6] if i < 6 else _elem(rng, "mix")           # both operands extreme where all six coefficients are
        out.append((a, ra, b, rb))
    if binary:
        out += [(b, rb, a, ra) for a, ra, b, rb in out[-len(ext) + 6:]]     # and the extreme coefficient in the second operand
    edge = pc.edge_f12()
    for i, e in enumerate(edge):
        o = edge[(i + 5) % len(edge)]
        for k in (0, 1):
            out.append((e, fr.raw_f12(e, k), o, fr.raw_f12(o, k)))
    return out


def _run(gpu, op, recs):
    assert 0 < len(recs) < 1000
    return gpu.fq12_raw_op(fr.OPS[op], np.stack(recs))


REFERENCE = {
    "mul": lambda a, b: pr.f12_mul(a, b),
    "sqr": lambda a, b: pr.f12_sqr(a),
    "sparse": lambda a, b: pr.f12_mul_sparse(a, (b[0], b[1], b[3])),
    "conj": lambda a, b: pr.f12_conj(a),
    "frob1": lambda a, b: pr.f12_frob(a, 1),
    "frob2": lambda a, b: pr.f12_frob(a, 2),
    "frob3": lambda a, b: pr.f12_frob(a, 3),
    "inv": lambda a, b: pr.f12_inv(a),
    "xi_mul": lambda a, b: [pr.xi_mul(c) for c in a],
}


@pytest.mark.parametrize("op", list(REFERENCE))
def test_operations_at_every_representative(gpu, op):
    """ops 0 .. 7 and 11: every component of both operands at k = 0, at k = 1, 200 random mixes of k and limb shape, the extreme
    vectors (all coefficients, one coefficient), the edge elements at both k.  The sparse product's three line coefficients are
    coefficients 0, 1, 3 of the second operand and get the same treatment; the product and the square are also held to the oracle's
    f12_mul, the inverse to x x^-1 = 1."""
    rng = _rng("ops", op)
    cases = _operands(rng, op in ("mul", "sparse"))
    out = _run(gpu, op, [fr.record(ra, rb) for _, ra, _, rb in cases])
    for i, (a, _, b, _) in enumerate(cases):
        want = REFERENCE[op](a, b)
        fr.check(out[i], want, f"{op} case {i}")
        if op == "mul":
            assert want == bp.f12_mul(a, b)
        elif op == "sqr":
            assert want == bp.f12_mul(a, a)
        elif op == "inv":
            assert bp.f12_mul(a, fr.residues(out[i])) == (pc.ONE if a != ZERO12 else ZERO12), f"inv case {i}"


def test_to_wire_gives_the_canonical_words_of_every_representative(gpu):
    """op 12: q2::to_wire of every coefficient -- eight canonical Montgomery words per component, the ninth 0"""
    rng = _rng("to_wire")
    cases = _operands(rng, False)
    out = _run(gpu, "to_wire", [fr.record(ra) for _, ra, _, _ in cases])
    for i, (a, _, _, _) in enumerate(cases):
        assert np.array_equal(out[i], fr.wire_words(a)), f"to_wire case {i}"


def test_inverse_of_every_representative_of_zero(gpu):
    """f12_inv(0) = 0 rests on fq_inv(0) = 0 and on N = 0 being recognised as a product of zeros whatever multiple of M stands for
    them: every coefficient at each of the four (k, k') of (0, 0), the others at random k; all at k = 0; all at k = 1"""
    rng = _rng("inv-zero")
    recs = [fr.raw_f12(ZERO12, 0), fr.raw_f12(ZERO12, 1)]
    for i in range(6):
        for k in range(2):
            for k2 in range(2):
                ks = [int(rng.integers(0, 2)) for _ in range(12)]
                ks[2 * i], ks[2 * i + 1] = k, k2
                recs.append(fr.raw_f12(ZERO12, ks))
    assert all(fr.residues(r) == ZERO12 for r in recs) and any(r.any() for r in recs)
    out = _run(gpu, "inv", [fr.record(r) for r in recs])
    for i, row in enumerate(out):
        fr.check(row, ZERO12, f"inverse of zero, representative {i}")


@pytest.fixture(scope="module")
def cyclotomic():
    """elements of the cyclotomic subgroup: easy parts of random elements, and 1"""
    rnd = random.Random("fq12-raw-cyclotomic")
    return [pr.easy_part(pc.rand_f12(rnd)) for _ in range(6)] + [list(pc.ONE)]


def _cyc_cases(rng, cyclotomic, mixes):
    return [(g, _reps(rng, g, mode)) for g in cyclotomic for mode in ["min", "max"] + ["mix"] * mixes]


def test_cyclotomic_square_equals_the_plain_square(gpu, cyclotomic):
    """op 8 on the cyclotomic subgroup (inputs vary in k and limb shape only): the residues of the plain square"""
    rng = _rng("cyc")
    cases = _cyc_cases(rng, cyclotomic, 6)
    out = _run(gpu, "cyc", [fr.record(r) for _, r in cases])
    for i, (g, _) in enumerate(cases):
        want = pr.f12_sqr(g)
        assert want == pr.f12_cyc_sqr(g) == bp.f12_mul(g, g)
        fr.check(out[i], want, f"cyc case {i}")


def test_easy_part_of_every_representative(gpu, cyclotomic):
    """op 9 (conj, inverse, Frobenius, two products): inputs from the cyclotomic subgroup, k and limb shape vary"""
    rng = _rng("easy")
    cases = _cyc_cases(rng, cyclotomic[:3], 2)
    out = _run(gpu, "easy", [fr.record(r) for _, r in cases])
    want = {id(g): pr.easy_part(g) for g in cyclotomic[:3]}
    for i, (g, _) in enumerate(cases):
        fr.check(out[i], want[id(g)], f"easy case {i}")


def test_hard_part_of_every_representative(gpu, cyclotomic):
    """op 10: three inputs of the cyclotomic subgroup at k = 0, at k = 1 and mixed -- some 200 loop-carried Granger-Scott squares and
    70 products each, every one fed the raw output of the one before"""
    rng = _rng("hard")
    gs = cyclotomic[:3]
    recs = [_reps(rng, g, mode) for g, mode in zip(gs, ("min", "max", "mix"))]
    out = _run(gpu, "hard", [fr.record(r) for r in recs])
    for i, g in enumerate(gs):
        fr.check(out[i], pr.hard_part(g), f"hard case {i}")


@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_sizes_around_a_workgroup(gpu, n):
    """one workgroup holds eight elements: a single group with seven running along on element 0, one group short, a full workgroup, and
    a second workgroup with one live group (every barrier is still reached by every lane; nothing is written past n)"""
    rng = _rng("sizes", n)
    cases = [_elem(rng, "mix") + _elem(rng, "mix") for _ in range(n)]
    out = _run(gpu, "mul", [fr.record(ra, rb) for _, ra, _, rb in cases])
    assert out.shape == (n, fr.EL_WORDS)
    for i, (a, _, b, _) in enumerate(cases):
        fr.check(out[i], pr.f12_mul(a, b), f"n = {n} element {i}")


# ---- the Miller loop's steps ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_states():
    """(T, Q, P) with T the state of pairing_ref.miller_loop after its first steps: Q = 2 H, 3 H, 5 H, P = G, 2 G, 3 G"""
    hs = pc.h_multiples(5)
    out = []
    for q, p in ((hs[1], opy.G1_GEN), (hs[2], opy.g1_mul(opy.G1_GEN, 2)), (hs[4], opy.g1_mul(opy.G1_GEN, 3))):
        t = (q[0], q[1], (1, 0))
        for bit in bin(pr.ATE_LOOP)[3:9]:
            t, _ = pr.dbl_step(t)
            out.append((t, q, p))
            if bit == "1":
                t, _ = pr.add_step(t, q)
                out.append((t, q, p))
    return out


def _scaled(rng, t):
    """the same projective point under another factor of Fq2"""
    s = (_fq(rng) or 1, _fq(rng))
    return tuple(bp.f2_mul(c, s) for c in t)


def _step_ks(rng, mode):
    if mode in ("min", "max"):
        return [int(mode == "max")] * 10, [False] * 10
    return [int(rng.integers(0, 2)) for _ in range(10)], [bool(rng.integers(0, 2)) for _ in range(10)]


def _step_want(op, t, q, p):
    t3, co = pr.dbl_step(t) if op == "dbl" else pr.add_step(t, q)
    return t3, pr.line_at(co, p)


@pytest.mark.parametrize("op", ["dbl", "add"])
def test_miller_steps_at_every_representative(gpu, loop_states, op):
    """dbl_step and add_step on T from a real loop state under a random Fq2 factor: T and Q at every component's k = 0, k = 1 and 60
    mixes of k and limb shape; xP and -yP at each of their sixteen (k, k'), k = 0 .. 3.  T3 exact, l0 and l1 the coefficient times -yP
    resp. xP as line_at gives them, l3 exact; every lane of the group agrees."""
    rng = _rng("step", op)
    recs, want = [], []
    for i, mode in enumerate(["min", "max"] + ["mix"] * 60):
        for kb in ((i % 4, (i // 4) % 4), (3, 3)) if mode != "mix" else ((i % 4, (i // 4) % 4),):
            t, q, p = loop_states[i % len(loop_states)]
            t = _scaled(rng, t)
            ks, sl = _step_ks(rng, mode)
            row = fr.step_record(t, q, p[0], P - p[1], ks, sl, kb)
            assert fr.step_inputs_in_type(row)
            recs.append(row)
            want.append(_step_want(op, t, q, p))
    assert len({tuple(fr.value(l) // P for l in fr.components(r)[10:]) for r in recs}) == 16      # every (k, k') of the base operands
    out = gpu.miller_step_raw(int(op == "add"), np.stack(recs))
    for i, row in enumerate(out):
        fr.check_step(row, want[i][0], want[i][1], f"{op}_step case {i}")


def test_add_step_of_the_point_itself_and_of_its_negative(gpu, loop_states):
    """add_step with T = Q and T = -Q under a non-trivial z (lambda = 0; theta = 0 resp. 2 y z): the loop never meets these on
    subgroup points, but the formulas' residues, zeros included, are still what must come out, inside El, from differences that are
    multiples of M rather than 0"""
    rng = _rng("step-same")
    recs, want = [], []
    for i, mode in enumerate(["min", "max"] + ["mix"] * 10):
        _, q, p = loop_states[i % len(loop_states)]
        for sign in (1, -1):
            z = (_fq(rng) or 1, _fq(rng) or 1)
            t = (bp.f2_mul(q[0], z), bp.f2_mul(bp.f2_scale(q[1], sign % P), z), z)
            ks, sl = _step_ks(rng, mode)
            recs.append(fr.step_record(t, q, p[0], P - p[1], ks, sl, (i % 4, 3 - i % 4)))
            t3, line = _step_want("add", t, q, p)
            assert t3[0] == (0, 0) and t3[2] == (0, 0) and line[0] == (0, 0) and (sign == 1) == (line[1] == (0, 0))
            want.append((t3, line))
    out = gpu.miller_step_raw(1, np.stack(recs))
    for i, row in enumerate(out):
        fr.check_step(row, want[i][0], want[i][1], f"add_step T = +-Q case {i}")
