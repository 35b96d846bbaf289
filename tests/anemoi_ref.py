"""Anemoi-Jive over BN254's scalar field (AnemoiJive254: 2 columns, 14 rounds, alpha = 5, g = 5) restated on Python integers: the
permutation AND ITS INVERSE, the rate-3 sponge (eval_variable_length_hash, eval_stream_cipher) with the traces the circuits take
as their witness, and the twelve-element challenge of the zk-friendly reveal (chaum_pedersen/dl.rs prove0 / verify0).

Nothing is copied from a table: the 56 round keys follow the published rule
    C[i][j] = g pi0^(2 i) + (pi0^i + pi1^j)^5          D[i][j] = g pi1^(2 j) + (pi0^i + pi1^j)^5 + delta
over the two 100-digit blocks of pi's decimals that the Anemoi paper fixes, delta = 1 / g, and the S-box exponent is
5^-1 mod (r - 1).  tests/golden/anemoi_golden.json (the reference's recorded answers) pins the result.

The fifth root.  The open Flystel's inverse needs x^(1/5) as much as the forward direction does (t = x - g y^2 - delta, then
y + t^(1/5)), so the inverse cannot avoid the root; what makes both directions independent of the 254-bit exponent is that EVERY root
taken here is checked by a fifth power (u^5 == t: x -> x^5 is a bijection of the field, so u is the only answer) -- a wrong exponent
cannot pass, whatever the device computes with.
"""
from __future__ import annotations

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
ED_ORDER = 2736030358979909402780800718157159386076813972158567259200215660948447373041
ROUNDS, G, ALPHA, RATE = 14, 5, 5, 3
DELTA = pow(G, -1, R)
ALPHA_INV = pow(ALPHA, -1, R - 1)
PI0 = 1415926535897932384626433832795028841971693993751058209749445923078164062862089986280348253421170679
PI1 = 8214808651328230664709384460955058223172535940812848111745028410270193852110555964462294895493038196
MAX_INPUT, MAX_OUTPUT = 96, 96


def round_keys():
    c = [[(G * pow(PI0, 2 * i, R) + pow(pow(PI0, i, R) + pow(PI1, j, R), ALPHA, R)) % R for j in range(2)] for i in range(ROUNDS)]
    d = [[(G * pow(PI1, 2 * j, R) + pow(pow(PI0, i, R) + pow(PI1, j, R), ALPHA, R) + DELTA) % R for j in range(2)] for i in range(ROUNDS)]
    return c, d


KEYS_X, KEYS_Y = round_keys()


def fifth_root(t):
    u = pow(t, ALPHA_INV, R)
    assert pow(u, ALPHA, R) == t % R, "the S-box exponent is not 1/5"
    return u


def mds(x, y):
    """[[1, g], [g, g^2 + 1]] on x as it is, on y after swapping its two words."""
    x0, x1 = x
    y0, y1 = y[1], y[0]
    return [(x0 + G * x1) % R, (G * x0 + (G * G + 1) * x1) % R], [(y0 + G * y1) % R, (G * y0 + (G * G + 1) * y1) % R]


def mds_inverse(x, y):
    # det = (g^2 + 1) - g^2 = 1: the inverse is [[g^2 + 1, -g], [-g, 1]]
    x0, x1 = x
    y0, y1 = y
    ix = [((G * G + 1) * x0 - G * x1) % R, (x1 - G * x0) % R]
    iy = [((G * G + 1) * y0 - G * y1) % R, (y1 - G * y0) % R]
    return ix, [iy[1], iy[0]]


def linear(x, y):
    x, y = mds(x, y)
    y = [(y[i] + x[i]) % R for i in range(2)]
    x = [(x[i] + y[i]) % R for i in range(2)]
    return x, y


def linear_inverse(x, y):
    x = [(x[i] - y[i]) % R for i in range(2)]
    y = [(y[i] - x[i]) % R for i in range(2)]
    return mds_inverse(x, y)


def sbox(x, y):
    t = (x - G * y * y) % R
    y = (y - fifth_root(t)) % R
    return (t + G * y * y + DELTA) % R, y


def sbox_inverse(x, y):
    t = (x - G * y * y - DELTA) % R
    y = (y + fifth_root(t)) % R
    return (t + G * y * y) % R, y


def permute_with_trace(state):
    """state = [x0, x1, y0, y1] -> (after, the 14 x [x0, x1, y0, y1] after each round's S-box)."""
    x, y = [state[0] % R, state[1] % R], [state[2] % R, state[3] % R]
    mid = []
    for r in range(ROUNDS):
        x = [(x[i] + KEYS_X[r][i]) % R for i in range(2)]
        y = [(y[i] + KEYS_Y[r][i]) % R for i in range(2)]
        x, y = linear(x, y)
        for i in range(2):
            x[i], y[i] = sbox(x[i], y[i])
        mid.append(x + y)
    x, y = linear(x, y)
    return x + y, mid


def permute(state):
    return permute_with_trace(state)[0]


def permute_inverse(state, from_round=ROUNDS):
    """The state before the permutation from the one after it; with from_round = k < 14, `state` is taken as the state after the S-box
    of round k - 1 (what round k starts from), so the result is the input whose round k begins there."""
    x, y = [state[0] % R, state[1] % R], [state[2] % R, state[3] % R]
    if from_round == ROUNDS:
        x, y = linear_inverse(x, y)
    for r in range(from_round - 1, -1, -1):
        for i in range(2):
            x[i], y[i] = sbox_inverse(x[i], y[i])
        x, y = linear_inverse(x, y)
        x = [(x[i] - KEYS_X[r][i]) % R for i in range(2)]
        y = [(y[i] - KEYS_Y[r][i]) % R for i in range(2)]
    return x + y


def state_with_sbox_input(rnd, column, value, other=None):
    """An input state whose round `rnd` feeds exactly `value` (0 or 1: where an exponentiation chain most plausibly goes wrong) into the
    fifth root of `column`.  other: the remaining three free words at that point (y of both columns and the other column's root input)."""
    y0, y1, t_other = other if other is not None else (0x1234567 + rnd, 0x7654321 + 3 * column, 0xabcdef + rnd)
    ys = [y0 % R, y1 % R]
    ts = [t_other % R, t_other % R]
    ts[column] = value
    x = [(ts[i] + G * ys[i] * ys[i]) % R for i in range(2)]               # after the linear layer of round rnd
    x, y = linear_inverse(x, ys)
    x = [(x[i] - KEYS_X[rnd][i]) % R for i in range(2)]
    y = [(y[i] - KEYS_Y[rnd][i]) % R for i in range(2)]
    return permute_inverse(x + y, from_round=rnd)


def sbox_inputs(state):
    """The 14 x 2 values that enter the fifth root while `state` is permuted."""
    x, y = [state[0] % R, state[1] % R], [state[2] % R, state[3] % R]
    out = []
    for r in range(ROUNDS):
        x = [(x[i] + KEYS_X[r][i]) % R for i in range(2)]
        y = [(y[i] + KEYS_Y[r][i]) % R for i in range(2)]
        x, y = linear(x, y)
        out.append([(x[i] - G * y[i] * y[i]) % R for i in range(2)])
        for i in range(2):
            x[i], y[i] = sbox(x[i], y[i])
    return out


# ---- the sponge ------------------------------------------------------------------------------------------------------------------
def pad(inputs):
    """(padded input, sigma): a nonempty multiple of 3 is taken as it is with sigma = 1; anything else gets a 1, then zeros."""
    inputs = [v % R for v in inputs]
    if len(inputs) % RATE == 0 and inputs:
        return inputs, 1
    inputs = inputs + [1]
    inputs += [0] * (-len(inputs) % RATE)
    return inputs, 0


def permutations(length, out_len=0):
    """How many permutations one item runs (uzk_anemoi_permutations); out_len = 0: a hash."""
    absorb = length // RATE if (length % RATE == 0 and length > 0) else length // RATE + 1
    if out_len <= RATE:
        return absorb
    return absorb + out_len // RATE - 1 + (1 if out_len % RATE else 0)


class Trace:
    """before / after: P x [x0, x1, y0, y1]; mid: P x 14 x [x0, x1, y0, y1] (intermediate_values_before_constant_additions)."""

    def __init__(self):
        self.before, self.mid, self.after, self.output = [], [], [], None

    def flat(self):
        """The layout of the C ABI's trace_out: per permutation before (4), the 14 rounds (56), after (4)."""
        out = []
        for b, m, a in zip(self.before, self.mid, self.after):
            out += list(b)
            for row in m:
                out += list(row)
            out += list(a)
        return out


def _sponge(inputs, out_len, sigma_override=None):
    padded, sigma = pad(inputs)
    if sigma_override is not None:
        sigma = sigma_override
    tr = Trace()
    st = [0, 0, 0, 0]

    def run():
        nonlocal st
        tr.before.append(list(st))
        st, mid = permute_with_trace(st)
        tr.mid.append(mid)
        tr.after.append(list(st))

    for k in range(0, len(padded), RATE):
        st = [(st[0] + padded[k]) % R, (st[1] + padded[k + 1]) % R, (st[2] + padded[k + 2]) % R, st[3]]
        run()
    st[3] = (st[3] + sigma) % R
    if out_len is None:
        tr.output = st[0]
        return tr
    out = []
    if out_len <= RATE:
        out = st[:out_len]
    else:
        out = st[:RATE]
        for _ in range(out_len // RATE - 1):
            run()
            out += st[:RATE]
        if out_len % RATE:
            run()
            out += st[:out_len % RATE]
    tr.output = out
    return tr


def eval_variable_length_hash_with_trace(inputs):
    return _sponge(inputs, None)


def eval_variable_length_hash(inputs):
    return _sponge(inputs, None).output


def eval_stream_cipher_with_trace(inputs, out_len, sigma_override=None):
    return _sponge(inputs, out_len, sigma_override)


def eval_stream_cipher(inputs, out_len, sigma_override=None):
    return _sponge(inputs, out_len, sigma_override).output


# ---- the zk-friendly reveal's challenge --------------------------------------------------------------------------------------------
def point_words(p):
    """A point as dl.rs feeds it to the hash: into_affine().xy().unwrap_or_default().  Upstream arkworks' xy() is None for the identity,
    which would enter as (0, 0), not (0, 1) -- SUPPOSED from upstream, the reference's fork could not be read."""
    x, y = p
    return (0, 0) if (x % R, y % R) == (0, 1) else (x % R, y % R)


def cp0_challenge(g, h, u, v, a, b):
    """c of prove0 / verify0: the hash of the twelve coordinates as an integer below r, reduced mod the subgroup order."""
    words = []
    for p in (g, h, u, v, a, b):
        words += list(point_words(p))
    return eval_variable_length_hash(words) % ED_ORDER


def prove0(sk, e1, omega):
    """ed_ref.prove with the zk-friendly challenge: (reveal card, proof blob)"""
    import ed_ref as e
    reveal, pk = e.mul(sk, e1), e.mul(sk, e.G)
    a, b = e.mul(omega, e1), e.mul(omega, e.G)
    c = cp0_challenge(e1, e.G, reveal, pk, a, b)
    return reveal, e.make_proof(a, b, (omega + c * sk) % e.L)


def verify0(statement, blob, want_challenge=False):
    """ed_ref.verify with the zk-friendly challenge: the same verdict codes in the same order"""
    import ed_ref as e
    a, b, r = e.parse_proof(blob)
    e1, reveal, pk = (statement[0], statement[1]), (statement[2], statement[3]), (statement[4], statement[5])
    pts = (e1, reveal, pk, a, b)
    if any(v >= e.Q for p in pts for v in p):
        st = e.NOT_CANONICAL
    elif not all(e.on_curve(p) for p in pts):
        st = e.OFF_CURVE
    else:
        st = max(e.classify(p) for p in pts)
    c = None
    if st == e.OK:
        c = cp0_challenge(e1, e.G, reveal, pk, a, b)
        if not e.peq(e.pmul(r, e1), e.padd(e.proj(a), e.pmul(c, reveal))):
            st = e.EQ1_FAILS
        elif not e.peq(e.pmul(r, e.G), e.padd(e.proj(b), e.pmul(c, pk))):
            st = e.EQ2_FAILS
    return (st, c) if want_challenge else st


# ---- the golden cases and the wire -------------------------------------------------------------------------------------------------
def golden():
    import json
    import os
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anemoi_golden.json")))
    return {"input": [int(v) for v in g["input"]], "hash": int(g["hash"]), "stream": [int(v) for v in g["stream_cipher"]["output"]],
            "lengths": [int(v) for v in g["stream_cipher"]["compared_at_lengths"]]}


def wire(vals):
    """integers below r -> n x 4 uint64 Montgomery words"""
    import ed_ref as e
    return e.fr_wire(vals)


def unwire(a):
    import ed_ref as e
    return e.fr_unwire(a)
