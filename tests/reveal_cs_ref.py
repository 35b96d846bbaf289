"""CPU restatement, on Python integers, of the R1CS a Groth16 reveal proof is made over: RevealCircuit of
shuffle/src/reveal_with_snark.rs with ark-r1cs-std 0.4's twisted Edwards gadget (EdwardsVar over ark_ed_on_bn254, a = 1), synthesised the
way ark-relations does it: field variables are constants or linear combinations, a product of two variables allocates a witness and a row.

  instance    1, h.x, h.y, reveal.x, reveal.y, pk.x, pk.y                                    (l = 7; h = masked.e1)
  points      each input point: x2 = x x, y2 = y y, (d x2 - 1) y2 = a x2 - 1                  2 witnesses, 3 rows
  bits        256 little-endian bits of sk: (1 - b) b = 0
  fixed       g.scalar_mul_le(sk): res = 0, multiple = 2^i G (constants); per bit tmp = res + multiple, res = bit.select(tmp, res).
              Iteration 0 is linear in the bit; iterations 1 .. 255: v0v1, x3, y3, sel_x, sel_y  (5 witnesses, 5 rows), then
              res == pk (2 rows)
  variable    h.scalar_mul_le(sk): iteration 0 adds to the constant neutral point (v0v1, x3, y3), selects (2) and doubles
              (xy, x2, y2, x3, y3); iterations 1 .. 255: u, v0, v1, v0v1, x3, y3, sel_x, sel_y, xy, x2, y2, dx3, dy3
              (13 witnesses, 13 rows), then res == reveal (2 rows)

4869 variables, 4869 rows, domain 8192.  A row is a list of (column, value) sorted by column, zero coefficients dropped.
Every witness carries (chain, iteration, role); csrc/revealcs_layout.hpp has the same codes."""
import ed_ref as ed

Q, D, G = ed.Q, ed.D, ed.G
A_COEFF = 1
BITS = 256
N_INPUTS, N_VARS, N_CONSTRAINTS, DOMAIN = 7, 4869, 4869, 8192
CH_POINT, CH_BIT, CH_FIXED, CH_VAR = range(4)
# roles: CH_POINT x2 y2 (iteration = the point: 0 h, 1 reveal, 2 pk); CH_BIT bit; the chains as below
(R_X2, R_Y2, R_BIT, R_U, R_V0, R_V1, R_V0V1, R_X3, R_Y3, R_SELX, R_SELY, R_XY, R_DX2, R_DY2, R_DX3, R_DY3) = range(16)
ROLE_NAMES = ["x2", "y2", "bit", "u", "v0", "v1", "v0v1", "x3", "y3", "sel_x", "sel_y", "xy", "dx2", "dy2", "dx3", "dy3"]
OFF_POINTS, OFF_BITS, OFF_FIXED, OFF_VAR = 7, 13, 269, 1544       # first variable of each section


class Fp:
    """FpVar: Constant (lc is None) or Var (a linear combination {variable: coefficient}, variable 0 = one)"""

    def __init__(self, val, lc=None):
        self.val, self.lc = val % Q, lc

    @property
    def const(self):
        return self.lc is None

    def row(self):
        lc = {0: self.val} if self.const else self.lc
        return sorted((c, v % Q) for c, v in lc.items() if v % Q)


_VAR = {}                  # the combination of every Var while only values are wanted (witness): no rows are written then
_values_only = [False]


def _lin(x, kx, y=None, ky=0):
    """kx x + ky y"""
    val = x.val * kx + (y.val * ky if y is not None else 0)
    if x.const and (y is None or y.const):
        return Fp(val)
    if _values_only[0]:
        return Fp(val, _VAR)
    lc = {}
    for t, k in ((x, kx), (y, ky)):
        if t is None:
            continue
        for c, v in ({0: t.val} if t.const else t.lc).items():
            lc[c] = (lc.get(c, 0) + k * v) % Q
    return Fp(val, lc)


class CS:
    def __init__(self):
        self.A, self.B, self.C, self.z, self.roles = [], [], [], [1], {}
        self.one = Fp(1)

    def new_var(self, val, role=None):
        self.z.append(val % Q)
        i = len(self.z) - 1
        if role is not None:
            self.roles[i] = role
        return Fp(val, _VAR if _values_only[0] else {i: 1})

    def enforce(self, a, b, c):
        if _values_only[0]:
            return
        self.A.append(a.row()); self.B.append(b.row()); self.C.append(c.row())

    def add(self, x, y):
        return _lin(x, 1, y, 1)

    def sub(self, x, y):
        return _lin(x, 1, y, -1)

    def scale(self, x, k):
        return _lin(x, k)

    def addc(self, x, k):
        return _lin(x, 1, self.one, k)

    def mul(self, x, y, role):
        if x.const or y.const:
            if x.const and y.const:
                return Fp(x.val * y.val)
            v, k = (y, x.val) if x.const else (x, y.val)
            if _values_only[0]:
                return Fp(v.val * k, _VAR)
            return Fp(v.val * k, {c: w * k % Q for c, w in v.lc.items()})          # stays a Var, also for k = 0
        w = self.new_var(x.val * y.val, role)
        self.enforce(x, y, w)
        return w

    def mul_equals(self, x, y, res):
        assert not (x.const or y.const or res.const)
        self.enforce(x, y, res)

    def select(self, bit, t, f, role):
        if t.const and f.const:
            return _lin(bit, t.val - f.val, self.one, f.val)                        # cond t + (1 - cond) f
        r = self.new_var(t.val if bit.val else f.val, role)
        self.enforce(bit, self.sub(t, f), self.sub(r, f))
        return r

    def enforce_equal(self, x, y):
        self.enforce(self.sub(x, y), self.one, Fp(0))


def _input_point(cs, p, k):
    x, y = p
    x2 = cs.mul(x, x, (CH_POINT, k, R_X2))
    y2 = cs.mul(y, y, (CH_POINT, k, R_Y2))
    cs.mul_equals(cs.addc(cs.scale(x2, D), -1), y2, cs.addc(cs.scale(x2, A_COEFF), -1))


def _add(cs, this, other, chain, it):
    if all(c.const for c in this + other):
        return tuple(Fp(v) for v in ed.add((this[0].val, this[1].val), (other[0].val, other[1].val)))
    u = cs.mul(cs.add(cs.scale(this[0], -A_COEFF), this[1]), cs.add(other[0], other[1]), (chain, it, R_U))
    v0 = cs.mul(other[1], this[0], (chain, it, R_V0))
    v1 = cs.mul(other[0], this[1], (chain, it, R_V1))
    v2 = cs.scale(cs.mul(v0, v1, (chain, it, R_V0V1)), D)
    x3 = cs.new_var((v0.val + v1.val) * pow(1 + v2.val, -1, Q), (chain, it, R_X3))
    cs.mul_equals(x3, cs.addc(v2, 1), cs.add(v0, v1))
    y3 = cs.new_var((u.val + A_COEFF * v0.val - v1.val) * pow(1 - v2.val, -1, Q), (chain, it, R_Y3))
    cs.mul_equals(y3, cs.scale(cs.addc(v2, -1), -1), cs.sub(cs.add(u, cs.scale(v0, A_COEFF)), v1))
    return x3, y3


def _double(cs, p, chain, it):
    x, y = p
    if x.const and y.const:
        return tuple(Fp(v) for v in ed.add((x.val, y.val), (x.val, y.val)))
    xy = cs.mul(x, y, (chain, it, R_XY))
    x2 = cs.mul(x, x, (chain, it, R_DX2))
    y2 = cs.mul(y, y, (chain, it, R_DY2))
    ax2 = cs.scale(x2, A_COEFF)
    s = cs.add(ax2, y2)
    x3 = cs.new_var(2 * xy.val * pow(s.val, -1, Q), (chain, it, R_DX3))
    cs.mul_equals(x3, s, cs.scale(xy, 2))
    y3 = cs.new_var((y2.val - ax2.val) * pow(2 - s.val, -1, Q), (chain, it, R_DY3))
    cs.mul_equals(y3, cs.addc(cs.scale(s, -1), 2), cs.sub(y2, ax2))
    return x3, y3


def _scalar_mul_le(cs, base, bits, chain):
    res, multiple = (Fp(0), Fp(1)), base
    for it, bit in enumerate(bits):
        tmp = _add(cs, res, multiple, chain, it)
        res = (cs.select(bit, tmp[0], res[0], (chain, it, R_SELX)), cs.select(bit, tmp[1], res[1], (chain, it, R_SELY)))
        multiple = _double(cs, multiple, chain, it)
    return res


def synthesize(sk, e1, values_only=False):
    """the constraint system with the assignment of (sk, e1): e1 any curve point, 0 <= sk < 2^256.  values_only: the same walk with
    the linear combinations left out -- the assignment alone, several times faster"""
    assert 0 <= sk < 1 << BITS and ed.on_curve(e1)
    _values_only[0] = values_only
    try:
        return _synthesize(sk, e1)
    finally:
        _values_only[0] = False


def _synthesize(sk, e1):
    reveal, pk = ed.mul(sk, e1), ed.mul(sk, G)
    cs = CS()
    g = (Fp(G[0]), Fp(G[1]))
    pts = [(cs.new_var(p[0]), cs.new_var(p[1])) for p in (e1, reveal, pk)]
    for k, p in enumerate(pts):
        _input_point(cs, p, k)
    h, rv, pkv = pts
    bits = []
    for i in range(BITS):
        b = cs.new_var((sk >> i) & 1, (CH_BIT, i, R_BIT))
        cs.enforce(_lin(cs.one, 1, b, -1), b, Fp(0))
        bits.append(b)
    t1 = _scalar_mul_le(cs, g, bits, CH_FIXED)
    cs.enforce_equal(t1[0], pkv[0]); cs.enforce_equal(t1[1], pkv[1])
    t2 = _scalar_mul_le(cs, h, bits, CH_VAR)
    cs.enforce_equal(t2[0], rv[0]); cs.enforce_equal(t2[1], rv[1])
    return cs


_cache = {}


def system():
    """(A, B, C), roles: the matrices do not depend on the assignment"""
    if "cs" not in _cache:
        cs = synthesize(1, G)
        _cache["cs"] = ((cs.A, cs.B, cs.C), cs.roles)
    return _cache["cs"]


def matrices():
    return system()[0]


def roles():
    """{witness index: (chain, iteration, role)}"""
    return system()[1]


def witness(sk, e1):
    """the full assignment z[N_VARS], z[0] = 1"""
    return synthesize(sk, e1, values_only=True).z


def statement(sk, e1):
    """e1.x e1.y reveal.x reveal.y pk.x pk.y"""
    return witness_statement(witness(sk, e1))


def witness_statement(z):
    return tuple(z[1:7])


def satisfied(mats, z):
    dot = lambda row: sum(v * z[c] for c, v in row) % Q
    return [i for i, (a, b, c) in enumerate(zip(*mats)) if (dot(a) * dot(b) - dot(c)) % Q]


def columns(M):
    """{variable: {row: value}}"""
    out = {}
    for i, row in enumerate(M):
        for c, v in row:
            out.setdefault(c, {})[i] = v
    return out


def fixed_multiples():
    """2^i G, i < 256, affine"""
    out, p = [], G
    for _ in range(BITS):
        out.append(p)
        p = ed.add(p, p)
    return out
