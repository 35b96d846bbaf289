"""CPU restatement, on Python integers, of the circuit a zshuffle proof is made over: the slice of TurboCS that build_cs
(shuffle/src/build_cs.rs:26-55) drives, the indexer's evaluation vectors, extend_witness and verify_witness.

  TurboCS        uzkge/src/plonk/constraint_system/turbo/mod.rs: new() with its two constant gates, new_variable, insert_lc_gate,
                 linear_combine, insert_sub_gate / equal, prepare_pi_variable, attach_boolean_constraint_to_gate,
                 attach_shuffle_remark_constraints_to_gate, pad -- the same order of new_variable and finish_new_gate calls
  card           shuffle/mod.rs:64-85: variables e1.x, e1.y, e2.x, e2.y; CardVar = [e2.x, e2.y, e1.x, e1.y] (= Ciphertext::flatten)
  remark         shuffle/remark.rs:13-93: 84 x 4 trace variables, then 85 gates; the block row is recorded BEFORE the variables
  shuffle_card   shuffle/permutation.rs:10-215: matrix row-major, row sums (boolean rows), column sums, then per output row and
                 coordinate the products a c + b d in chunks of 2 followed by their sums in chunks of 3
  permutation    constraint_system/mod.rs:64-92 over the wire-major flattening, by buckets per variable instead of the quadratic scan
  tables         indexer.rs:301-478: s = k[perm / n] omega^(perm mod n), the nine selectors, qb, q_prk (zero), q_ecc = the marker of
                 the 84 constrained rows of every remark block (NOT selector 7), q_shuffle_generator / _public_key (turbo/mod.rs:310-364)
  witness        extend_witness: extended[w][row] = value[wiring[w][row]]; compute_witness_selectors (turbo/mod.rs:171-185)
  check          verify_witness (turbo/mod.rs:1041-1395): the four remark equations per block row, the gate equation, the boolean rows

For a deck of N cards: size = 2 + 89 N + 2 N (ceil(N/3) + 1) + 4 N (ceil(N/2) + ceil(ceil(N/2)/3)) + 4 N gates before the pad."""
import shuffle_ref as sr

R = sr.Q
ITER = sr.ITERATIONS
EDWARDS_A = 1
N_SEL, N_WIRES = 9, 5
MAX_CARDS = 64
# the order of the golden verifier keys' 32 commitments, and of every list of evaluation vectors here
KEY_ORDER = [("q", 9), ("s", 5), ("qb", 1), ("q_prk", 4), ("q_ecc", 1), ("q_shuffle_generator", 12)]


def gate_count(cards):
    h = -(-cards // 2)
    return 2 + 89 * cards + 2 * cards * (-(-cards // 3) + 1) + 4 * cards * (h + -(-h // 3)) + 4 * cards


class TurboCS:
    def __init__(self):
        self.selectors = [[] for _ in range(N_SEL)]
        self.wiring = [[] for _ in range(N_WIRES)]
        self.num_vars, self.size, self.witness = 2, 0, [0, 1]
        self.public_vars_constraint_indices, self.public_vars_witness_indices = [], []
        self.boolean_constraint_indices = []
        self.shuffle_remark_constraint_indices = []          # (row, [3][84] wire selectors)
        self.insert_constant_gate(0, 0)
        self.insert_constant_gate(1, 1)

    def _gate(self, q, wires):
        """q = (q1, q2, q3, q4, qm1, qm2, qc, q_ecc, qo)"""
        for s, v in zip(self.selectors, q):
            s.append(v % R)
        for w, v in zip(self.wiring, wires):
            assert v < self.num_vars
            w.append(v)
        self.size += 1

    def new_variable(self, value):
        self.num_vars += 1
        self.witness.append(value % R)
        return self.num_vars - 1

    def insert_constant_gate(self, var, constant):
        self._gate((0, 0, 0, 0, 0, 0, constant, 0, 1), [var] * 5)

    def insert_lc_gate(self, wires_in, wire_out, q1, q2, q3, q4):
        self._gate((q1, q2, q3, q4, 0, 0, 0, 0, 1), list(wires_in) + [wire_out])

    def linear_combine(self, wires_in, q1, q2, q3, q4):
        w = self.witness
        out = self.new_variable(w[wires_in[0]] * q1 + w[wires_in[1]] * q2 + w[wires_in[2]] * q3 + w[wires_in[3]] * q4)
        self.insert_lc_gate(wires_in, out, q1, q2, q3, q4)
        return out

    def equal(self, left, right):                            # insert_sub_gate(left, right, zero_var)
        self.insert_lc_gate([left, right, 0, 0], 0, 1, -1, 0, 0)

    def prepare_pi_variable(self, var):
        self.public_vars_witness_indices.append(var)
        self.public_vars_constraint_indices.append(self.size)
        self.insert_constant_gate(var, 0)

    def attach_boolean_constraint_to_gate(self):
        self.boolean_constraint_indices.append(self.size - 1)

    def sum_chunks(self, variables, boolean):
        """the running sum in chunks of 3 that shuffle_card writes out three times"""
        acc = 0
        for at in range(0, len(variables), 3):
            c = list(variables[at:at + 3])
            q = [1] * len(c) + [0] * (3 - len(c))
            acc = self.linear_combine([acc] + c + [0] * (3 - len(c)), 1, q[0], q[1], q[2])
            if boolean:
                self.attach_boolean_constraint_to_gate()
        return acc

    def new_card_variable(self, card):
        (x1, y1), (x2, y2) = card
        a, b, c, d = self.new_variable(x1), self.new_variable(y1), self.new_variable(x2), self.new_variable(y2)
        return [c, d, a, b]

    def prepare_pi_card_variable(self, card_var):
        for v in card_var:
            self.prepare_pi_variable(v)

    def eval_card_remark(self, trace, bits, input_var):
        """trace: 84 entries (c2.x, c2.y, c1.x, c1.y); bits: 84 entries [s1, s2, s3]"""
        assert len(trace) == len(bits) == ITER
        self.shuffle_remark_constraint_indices.append((self.size, [[b[i] % R for b in bits] for i in range(3)]))
        iv = [[self.new_variable(x) for x in values] for values in trace]
        zero = (0,) * N_SEL
        self._gate(zero, list(input_var) + [iv[0][3]])
        for r in range(ITER - 1):
            self._gate(zero, iv[r] + [iv[r + 1][3]])
        self._gate(zero, iv[ITER - 1] + [0])
        return list(iv[ITER - 1])

    def shuffle_card(self, card_vars, perm):
        n = len(perm)
        assert len(card_vars) == n
        matrix = [[self.new_variable(1 if perm[i] == j else 0) for j in range(n)] for i in range(n)]
        for row in matrix:
            self.equal(self.sum_chunks(row, True), 1)
        for j in range(n):
            self.equal(self.sum_chunks([matrix[i][j] for i in range(n)], False), 1)
        split = [[cv[i] for cv in card_vars] for i in range(4)]
        out, w = [], self.witness
        for row in matrix:
            card = []
            for coords in split:
                r_vars = []
                for at in range(0, n, 2):
                    p, c = row[at:at + 2], coords[at:at + 2]
                    if len(p) == 2:
                        rv = self.new_variable(w[p[0]] * w[c[0]] + w[p[1]] * w[c[1]])
                        self._gate((0, 0, 0, 0, 1, 1, 0, 0, 1), [p[0], c[0], p[1], c[1], rv])
                    else:
                        rv = self.new_variable(w[p[0]] * w[c[0]])
                        self._gate((0, 0, 0, 0, 1, 1, 0, 0, 1), [p[0], c[0], 0, 0, rv])
                    r_vars.append(rv)
                card.append(self.sum_chunks(r_vars, False))
            out.append(card)
        return out

    def pad(self):
        n = 1
        while n < self.size:
            n *= 2
        for s in self.selectors:
            s.extend([0] * (n - self.size))
        for w in self.wiring:
            w.extend([0] * (n - self.size))
        self.size = n


def digit_bits(d):
    """RemarkTrace::bits of one step (shuffle/remark.rs:163-222): [bit0, bit1, +-1]"""
    return [d & 1, (d >> 1) & 1, 1 if d & 4 else R - 1]


def build_cs(cards, digits=None, perm=None, t_pk=None):
    """build_cs for a deck of (e1, e2) cards.  digits None: the layout alone (every value zero, the identity permutation)."""
    n = len(cards)
    assert 1 <= n <= MAX_CARDS
    cs, remarked = TurboCS(), []
    for k, card in enumerate(cards):
        if digits is None:
            trace, bits = [(0, 0, 0, 0)] * ITER, [[0, 0, 1]] * ITER
        else:
            trace, bits = sr.eval_remark_with_trace(card, digits[k], t_pk), [digit_bits(d) for d in digits[k]]
        iv = cs.new_card_variable(card)
        cs.prepare_pi_card_variable(iv)
        remarked.append(cs.eval_card_remark(trace, bits, iv))
    out_vars = cs.shuffle_card(remarked, list(range(n)) if perm is None else list(perm))
    for cv in out_vars:
        cs.prepare_pi_card_variable(cv)
    cs.gates = cs.size
    cs.pad()
    cs.output_vars = out_vars
    return cs


def layout(cards):
    return build_cs([((0, 1), (0, 1))] * cards)


def compute_permutation(cs):
    n = cs.size
    flat = [v for w in cs.wiring for v in w]
    buckets = [[] for _ in range(cs.num_vars)]
    for i, v in enumerate(flat):
        buckets[v].append(i)
    perm = [0] * (N_WIRES * n)
    for b in buckets:
        for a, nxt in zip(b, b[1:] + b[:1]):
            perm[a] = nxt
    return perm


def domain(n, root):
    g, out = 1, []
    for _ in range(n):
        out.append(g)
        g = g * root % R
    assert g == 1 and out[n // 2] == R - 1
    return out


def remark_rows(cs):
    return [row for row, _ in cs.shuffle_remark_constraint_indices]


def table_columns(cs, entries):
    """compute_shuffle_generator_selectors / _public_key_selectors: 12 vectors, x of the four j, then y, then d x y"""
    cols = [[0] * cs.size for _ in range(12)]
    for row in remark_rows(cs):
        for j in range(ITER):
            for part in range(3):
                for e in range(4):
                    cols[4 * part + e][row + j] = entries[j][e][part]
    return cols


def key_vectors(cs, k, root, gen_entries=None):
    """The 32 evaluation vectors behind the verifier key, in KEY_ORDER."""
    n = cs.size
    group, perm = domain(n, root), compute_permutation(cs)
    s = [[k[p // n] * group[p % n] % R for p in perm[w * n:(w + 1) * n]] for w in range(N_WIRES)]
    qb, q_ecc = [0] * n, [0] * n
    for i in cs.boolean_constraint_indices:
        qb[i] = 1
    for row in remark_rows(cs):
        for j in range(ITER):
            q_ecc[row + j] = 1
    gen_entries = gen_entries or [[sr.entry(t) for t in row] for row in sr.generator_tables()]
    return [list(v) for v in cs.selectors] + s + [qb] + [[0] * n for _ in range(4)] + [q_ecc] + table_columns(cs, gen_entries)


def extend_witness(cs, witness=None):
    w = cs.witness if witness is None else witness
    return [[w[v] for v in wire] for wire in cs.wiring]


def witness_selectors(cs):
    polys = [[0] * cs.size for _ in range(3)]
    for row, sel in cs.shuffle_remark_constraint_indices:
        for j in range(ITER):
            for i in range(3):
                polys[i][row + j] = sel[i][j]
    return polys


def public_inputs(cs, witness=None):
    w = cs.witness if witness is None else witness
    return [w[v] for v in cs.public_vars_witness_indices]


def verify_witness(cs, witness, online, pk_entries, gen_entries=None):
    """None if the witness satisfies the circuit, else a sentence saying where it does not."""
    gen_entries = gen_entries or [[sr.entry(t) for t in row] for row in sr.generator_tables()]
    if len(witness) != cs.num_vars:
        return "witness length"
    if len(online) != len(cs.public_vars_witness_indices):
        return "wrong number of online variables"
    W, a_ed = cs.wiring, EDWARDS_A
    for row, sel in cs.shuffle_remark_constraint_indices:
        for r in range(ITER):
            a, b, c, d, o = (witness[W[i][row + r]] for i in range(5))
            an, bn, cn, dn = (witness[W[i][row + r + 1]] for i in range(4))
            if o != dn:
                return "row %d round %d: the output wire is not the next row's fourth wire" % (row, r)
            s1, s2, s3 = sel[0][r], sel[1][r], sel[2][r]
            if s1 not in (0, 1) or s2 not in (0, 1) or s3 not in (1, R - 1):
                return "row %d round %d: wire selectors out of range" % (row, r)
            eq = [0, 0, 0, 0]
            for e in range(4):
                wgt = (s1 if e & 1 else 1 - s1) * (s2 if e & 2 else 1 - s2)
                px, py, pd = pk_entries[r][e]
                gx, gy, gd = gen_entries[r][e]
                eq[0] += wgt * (s3 * an - s3 * a * py - b * px + a * b * an * pd)
                eq[1] += wgt * (s3 * bn + a_ed * a * px - s3 * b * py - a * b * bn * pd)
                eq[2] += wgt * (s3 * cn - s3 * c * gy - d * gx + c * d * cn * gd)
                eq[3] += wgt * (s3 * o + a_ed * c * gx - s3 * d * gy - c * d * o * gd)
            for i, v in enumerate(eq):
                if v % R:
                    return "row %d round %d: remark equation %d" % (row, r, i + 1)
    pi_at = {}
    for row, var, val in zip(cs.public_vars_constraint_indices, cs.public_vars_witness_indices, online):
        if witness[var] != val % R:
            return "row %d: online value does not match the witness" % row
        pi_at[row] = val % R
    booleans = set(cs.boolean_constraint_indices)
    for row in range(cs.size):
        w = [witness[W[i][row]] for i in range(5)]
        q = [cs.selectors[i][row] for i in range(N_SEL)]
        g = q[0] * w[0] + q[1] * w[1] + q[2] * w[2] + q[3] * w[3] + q[4] * w[0] * w[1] + q[5] * w[2] * w[3] + q[6] + pi_at.get(row, 0) + \
            q[7] * w[0] * w[1] * w[2] * w[3] * w[4] - q[8] * w[4]
        if g % R:
            return "row %d: gate equation" % row
        if row in booleans and any(v not in (0, 1) for v in w[1:4]):
            return "row %d: a boolean wire is not one or zero" % row
    return None
