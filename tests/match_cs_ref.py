"""CPU restatement, on Python integers over anemoi_ref.py, of the circuit a zmatchmaking proof is made over: build_cs
(matchmaking/src/build_cs.rs:27-66) for N players, 3 <= N <= 64, the indexer's evaluation vectors, extend_witness and verify_witness.

  TurboCS        uzkge/src/plonk/constraint_system/turbo/mod.rs: new() with its two constant gates, new_variable, insert_constant_gate,
                 insert_lc_gate / linear_combine / add, mul, select, prepare_pi_variable, the boolean and Anemoi attachments, pad --
                 the same order of new_variable and finish_new_gate calls
  anemoi         constraint_system/anemoi/mod.rs: a permutation is 56 variables (round r: x0 x1 y0 y1 after its S-box), 14 gates with
                 all-zero selectors and one gate per wanted output word.  The hash of one element is one permutation with a single
                 output gate.  The stream cipher takes the one-input-chunk path: for N <= 4 one output chunk; for N >= 5
                 ceil((N - 1) / 3) chunks, after the first permutation 4 after_permutation variables and one add gate (sigma = the zero
                 variable), before every middle permutation 4 new variables
  matchmaking    matchmaking.rs:42-229: the constants 2 .. N - 1, the hash, the cipher, then for i = 1 .. N - 1 the division of stream
                 output i - 1 (as a canonical integer) by i + 1, the one-hot bits of the remainder with their running sums (boolean rows),
                 the i + 1 gates index * bit = remainder * bit, the products bit * output with their running sums, and the i selects
  tables         indexer.rs:301-478: the nine selectors, s = k[perm / n] omega^(perm mod n), qb, and q_prk = the round keys after the
                 linear layer on rows a + r of every permutation block (turbo/mod.rs:285-304)
  check          verify_witness (turbo/mod.rs:1041-1395): the four Anemoi equations on each of the 14 rows of a block, the gate equation,
                 the boolean rows; check_copies: the copy constraints of an extended witness

Every variable carries a definition (kind, a, b, c): how its value follows from a match.  csrc/matchcs.hpp has the same kinds."""
import anemoi_ref as an

R = an.R
N_SEL, N_WIRES = 9, 5
MIN_PLAYERS, MAX_PLAYERS = 3, 64
ROUNDS = an.ROUNDS
# the order of the verifier key's commitments, and of every list of evaluation vectors here
KEY_ORDER = [("q", 9), ("s", 5), ("qb", 1), ("q_prk", 4)]
(CONST, INPUT, SEED, RANDOM, COMMIT, HASH_TRACE, STREAM_TRACE, STREAM_OUT, QUOT, REM, BIT, BIT_SUM, PRODUCT, PROD_SUM, SELECT) = range(15)
KIND_NAMES = ["const", "input", "seed", "random", "commit", "hash_trace", "stream_trace", "stream_out", "quot", "rem", "bit", "bit_sum",
              "product", "prod_sum", "select"]
M00, M01, M10, M11 = 1, an.G, an.G, an.G * an.G + 1                # the MDS matrix [[1, g], [g, g^2 + 1]]
PRK = [sum(an.linear(an.KEYS_X[r], an.KEYS_Y[r]), []) for r in range(ROUNDS)]      # [14][4]: prk1..4 of round r


def chunks_of(count):
    return -(-count // 3)


def stream_permutations(players):
    return 1 if players <= 4 else chunks_of(players - 1)


def gate_count(players):
    """gates before the pad: constants, the hash, the cipher, the N - 1 steps, the 2 N + 2 public inputs"""
    n, p = players, stream_permutations(players)
    steps = sum(3 * i + 4 + 2 * chunks_of(i + 1) for i in range(1, n))
    return n + 15 + (14 * p + (n - 1) + (1 if p > 1 else 0)) + steps + 2 * n + 2


def var_count(players):
    n, p = players, stream_permutations(players)
    steps = sum(3 * i + 5 + 2 * chunks_of(i + 1) for i in range(1, n))
    return 2 + n + 3 + (n - 2) + 56 + (n - 1) + (56 * p + (5 + 4 * (p - 2) if p > 1 else 0)) + steps


class TurboCS:
    def __init__(self):
        self.selectors = [[] for _ in range(N_SEL)]
        self.wiring = [[] for _ in range(N_WIRES)]
        self.num_vars, self.size, self.witness = 2, 0, [0, 1]
        self.defs = [(CONST, 0, 0, 0), (CONST, 1, 0, 0)]
        self.public_vars_constraint_indices, self.public_vars_witness_indices = [], []
        self.boolean_constraint_indices, self.anemoi_constraints_indices = [], []
        self.insert_constant_gate(0, 0)
        self.insert_constant_gate(1, 1)

    def _gate(self, q, wires):
        """q = (q1, q2, q3, q4, qm1, qm2, qc, q_ecc, qo), as small signed integers"""
        for s, v in zip(self.selectors, q):
            s.append(v)
        for w, v in zip(self.wiring, wires):
            assert v < self.num_vars
            w.append(v)
        self.size += 1

    def new_variable(self, value, definition):
        self.num_vars += 1
        self.witness.append(value % R)
        self.defs.append(tuple(definition) + (0,) * (4 - len(definition)))
        return self.num_vars - 1

    def insert_constant_gate(self, var, constant):
        self._gate((0, 0, 0, 0, 0, 0, constant, 0, 1), [var] * 5)

    def linear_combine(self, wires_in, q, definition):
        w = self.witness
        out = self.new_variable(sum(w[v] * c for v, c in zip(wires_in, q)), definition)
        self._gate(tuple(q) + (0, 0, 0, 0, 1), list(wires_in) + [out])
        return out

    def add(self, left, right, definition):
        return self.linear_combine([left, right, 0, 0], (1, 1, 0, 0), definition)

    def mul(self, left, right, definition):
        out = self.new_variable(self.witness[left] * self.witness[right], definition)
        self._gate((0, 0, 0, 0, 1, 0, 0, 0, 1), [left, right, 0, 0, out])
        return out

    def select(self, var0, var1, bit, definition):
        out = self.new_variable(self.witness[var0] if self.witness[bit] == 0 else self.witness[var1], definition)
        self._gate((0, 1, 0, 0, -1, 1, 0, 0, 1), [bit, var0, bit, var1, out])
        return out

    def prepare_pi_variable(self, var):
        self.public_vars_witness_indices.append(var)
        self.public_vars_constraint_indices.append(self.size)
        self.insert_constant_gate(var, 0)

    def sum_chunks(self, variables, boolean, kind, step):
        """the running sum in chunks of 3; the sum after the chunk that ends at entry `count` is the variable (kind, step, count)"""
        acc = 0
        for at in range(0, len(variables), 3):
            c = list(variables[at:at + 3])
            q = (1,) + (1,) * len(c) + (0,) * (3 - len(c))
            acc = self.linear_combine([acc] + c + [0] * (3 - len(c)), q, (kind, step, at + len(c)))
            if boolean:
                self.boolean_constraint_indices.append(self.size - 1)
        return acc

    def anemoi_permutation_round(self, x_var, y_var, outputs, mid, kind, perm):
        """outputs: [x0, x1, y0, y1] variables or None; mid: 14 x [x0, x1, y0, y1]; the variables are trace elements 4 + 4 r + c"""
        iv = [[self.new_variable(mid[r][c], (kind, perm, 4 + 4 * r + c)) for c in range(4)] for r in range(ROUNDS)]
        zero = (0,) * N_SEL
        self._gate(zero, [x_var[0], x_var[1], y_var[0], y_var[1], iv[0][3]])
        self.anemoi_constraints_indices.append(self.size - 1)
        for r in range(1, ROUNDS):
            self._gate(zero, iv[r - 1] + [iv[r][3]])
        rows = [(2 * M00, 2 * M01, M01, M00), (2 * M10, 2 * M11, M11, M10), (M00, M01, M01, M00), (M10, M11, M11, M10)]
        for var, q in zip(outputs, rows):
            if var is not None:
                self._gate(q + (0, 0, 0, 0, 1), iv[ROUNDS - 1] + [var])

    def pad(self):
        n = 1
        while n < self.size:
            n *= 2
        for s in self.selectors:
            s.extend([0] * (n - self.size))
        for w in self.wiring:
            w.extend([0] * (n - self.size))
        self.size = n


def build_cs(inputs, seed, random_number):
    """build_cs of one match: N = len(inputs) players, the committed seed and the random number."""
    n = len(inputs)
    assert MIN_PLAYERS <= n <= MAX_PLAYERS
    cs = TurboCS()
    input_vars = [cs.new_variable(v, (INPUT, i)) for i, v in enumerate(inputs)]
    random_var = cs.new_variable(random_number, (RANDOM,))
    hash_trace = an.eval_variable_length_hash_with_trace([seed])
    seed_var = cs.new_variable(seed, (SEED,))
    commit_var = cs.new_variable(hash_trace.output, (COMMIT,))
    # generate_constraints: the constants
    index_vars = [0, 1]
    for i in range(2, n):
        v = cs.new_variable(i, (CONST, i))
        cs.insert_constant_gate(v, i)
        index_vars.append(v)
    # the hash of the seed: the chunk (seed, 1, 0), one permutation, one output
    cs.anemoi_permutation_round([seed_var, 1], [0, 0], [commit_var, None, None, None], hash_trace.mid[0], HASH_TRACE, 0)
    # the stream cipher over (seed, random): the chunk (seed, random, 1), sigma = the zero variable
    st = an.eval_stream_cipher_with_trace([hash_trace.before[0][0], random_number], n - 1)
    out_vars = [cs.new_variable(v, (STREAM_OUT, i)) for i, v in enumerate(st.output)]
    padded = out_vars + [None] * (-len(out_vars) % 3)
    out_chunks = [padded[at:at + 3] + [None] for at in range(0, len(padded), 3)]
    assert len(out_chunks) == len(st.mid) == stream_permutations(n)
    x_var, y_var = [seed_var, random_var], [1, 0]
    cs.anemoi_permutation_round(x_var, y_var, out_chunks[0], st.mid[0], STREAM_TRACE, 0)
    if len(out_chunks) > 1:
        new = [cs.new_variable(st.after[0][c], (STREAM_TRACE, 0, 60 + c)) for c in range(4)]
        new[3] = cs.add(new[3], 0, (STREAM_TRACE, 0, 63))                # + sigma, the zero variable: the same value
        for rr in range(1, len(out_chunks)):
            x_var, y_var = new[:2], new[2:]
            if rr != len(out_chunks) - 1:
                new = [cs.new_variable(st.after[rr][c], (STREAM_TRACE, rr, 60 + c)) for c in range(4)]
            cs.anemoi_permutation_round(x_var, y_var, out_chunks[rr], st.mid[rr], STREAM_TRACE, rr)
    # the N - 1 steps
    outputs, w = list(input_vars), cs.witness
    for i in range(1, n):
        value = st.output[i - 1]
        quotient, remainder = divmod(value, i + 1)
        n_var = cs.new_variable(value, (STREAM_OUT, i - 1))
        q_var, r_var = cs.new_variable(quotient, (QUOT, i)), cs.new_variable(remainder, (REM, i))
        cs._gate((i + 1, 1, 0, 0, 0, 0, 0, 0, 1), [q_var, r_var, 0, 0, n_var])
        bits = [cs.new_variable(1 if j == remainder else 0, (BIT, i, j)) for j in range(i + 1)]
        total = cs.sum_chunks(bits, True, BIT_SUM, i)
        cs.insert_constant_gate(total, 1)
        for j in range(i + 1):
            cs._gate((0, 0, 0, 0, 1, -1, 0, 0, 0), [index_vars[j], bits[j], r_var, bits[j], 0])
        output_i = outputs[i]
        products = [cs.mul(bits[j], outputs[j], (PRODUCT, i, j)) for j in range(i + 1)]
        outputs[i] = cs.sum_chunks(products, False, PROD_SUM, i)
        for j in range(i):
            outputs[j] = cs.select(outputs[j], output_i, bits[j], (SELECT, i, j))
    # the public inputs: verify_matchmaking's online inputs
    for v in input_vars + outputs + [random_var, commit_var]:
        cs.prepare_pi_variable(v)
    cs.gates = cs.size
    cs.pad()
    cs.output_vars, cs.players = outputs, n
    return cs


def layout(players):
    """the circuit of gen_prover_params: the all-zero match"""
    return build_cs([0] * players, 0, 0)


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


def prk_rows(cs):
    """[n]: 0, or 1 + round on row a + round of a permutation block"""
    rows = [0] * cs.size
    for a in cs.anemoi_constraints_indices:
        for r in range(ROUNDS):
            rows[a + r] = 1 + r
    return rows


def key_vectors(cs, k, root):
    """The 19 evaluation vectors behind the verifier key, in KEY_ORDER."""
    n = cs.size
    group, perm = domain(n, root), compute_permutation(cs)
    s = [[k[p // n] * group[p % n] % R for p in perm[w * n:(w + 1) * n]] for w in range(N_WIRES)]
    qb = [0] * n
    for i in cs.boolean_constraint_indices:
        qb[i] = 1
    rows = prk_rows(cs)
    prk = [[PRK[r - 1][i] if r else 0 for r in rows] for i in range(4)]
    return [[v % R for v in sel] for sel in cs.selectors] + s + [qb] + prk


def extend_witness(cs, witness=None):
    w = cs.witness if witness is None else witness
    return [[w[v] for v in wire] for wire in cs.wiring]


def public_inputs(cs, witness=None):
    w = cs.witness if witness is None else witness
    return [w[v] for v in cs.public_vars_witness_indices]


def verify_witness(cs, witness, online):
    """None if the witness satisfies the circuit, else a sentence saying where it does not."""
    if len(witness) != cs.num_vars:
        return "witness length"
    if len(online) != len(cs.public_vars_witness_indices):
        return "wrong number of online variables"
    W, g, g_inv = cs.wiring, an.G, an.DELTA
    g2 = g * g + 1
    for a_row in cs.anemoi_constraints_indices:
        for r in range(ROUNDS):
            a, b, c, d, o = (witness[W[i][a_row + r]] for i in range(5))
            an_, bn, cn, dn = (witness[W[i][a_row + r + 1]] for i in range(4))
            if o != dn:
                return "row %d round %d: the output wire is not the next row's fourth wire" % (a_row, r)
            pa, pb, pc_, pd = PRK[r]
            da, cb = a + d, b + c
            d2a, c2b = da + a, cb + b
            e1 = da + g * cb + pc_
            e2 = g * da + g2 * cb + pd
            eqs = [pow(e1 - cn, 5, R) + g * e1 * e1 - (d2a + g * c2b + pa),
                   pow(e2 - dn, 5, R) + g * e2 * e2 - (g * d2a + g2 * c2b + pb),
                   pow(e1 - cn, 5, R) + g * cn * cn + g_inv - an_,
                   pow(e2 - dn, 5, R) + g * dn * dn + g_inv - bn]
            for i, v in enumerate(eqs):
                if v % R:
                    return "row %d round %d: anemoi equation %d" % (a_row, r, i + 1)
    pi_at = {}
    for row, var, val in zip(cs.public_vars_constraint_indices, cs.public_vars_witness_indices, online):
        if witness[var] != val % R:
            return "row %d: online value does not match the witness" % row
        pi_at[row] = val % R
    booleans = set(cs.boolean_constraint_indices)
    for row in range(cs.size):
        w = [witness[W[i][row]] for i in range(5)]
        q = [cs.selectors[i][row] for i in range(N_SEL)]
        gate = q[0] * w[0] + q[1] * w[1] + q[2] * w[2] + q[3] * w[3] + q[4] * w[0] * w[1] + q[5] * w[2] * w[3] + q[6] + pi_at.get(row, 0) + \
            q[7] * w[0] * w[1] * w[2] * w[3] * w[4] - q[8] * w[4]
        if gate % R:
            return "row %d: gate equation" % row
        if row in booleans and any(v not in (0, 1) for v in w[1:4]):
            return "row %d: a boolean wire is not one or zero" % row
    return None


def check_copies(cs, extended, perm=None):
    """None if every position of the extended witness [5][n] holds what the next position of its permutation cycle holds."""
    perm = compute_permutation(cs) if perm is None else perm
    flat = [v for wire in extended for v in wire]
    for p, nxt in enumerate(perm):
        if flat[p] != flat[nxt]:
            return "wire %d row %d: copy constraint" % (p // cs.size, p % cs.size)
    return None


def evaluate_defs(defs, inputs, seed, random_number):
    """Every variable's value from its definition alone: what the device computes per (match, variable)."""
    n = len(inputs)
    h = an.eval_variable_length_hash_with_trace([seed])
    st = an.eval_stream_cipher_with_trace([seed, random_number], n - 1)
    h_flat, s_flat = h.flat(), st.flat()
    rem = [0] + [st.output[i - 1] % (i + 1) for i in range(1, n)]
    state = [[], list(range(n))]                                         # state[i]: the index vector before step i
    for i in range(1, n):
        cur = list(state[i])
        cur[i], cur[rem[i]] = cur[rem[i]], cur[i]
        state.append(cur)
    out = []
    for kind, a, b, c in defs:
        if kind == CONST:
            v = a
        elif kind == INPUT:
            v = inputs[a]
        elif kind == SEED:
            v = seed
        elif kind == RANDOM:
            v = random_number
        elif kind == COMMIT:
            v = h.output
        elif kind == HASH_TRACE:
            v = h_flat[64 * a + b]
        elif kind == STREAM_TRACE:
            v = s_flat[64 * a + b]
        elif kind == STREAM_OUT:
            v = st.output[a]
        elif kind == QUOT:
            v = st.output[a - 1] // (a + 1)
        elif kind == REM:
            v = rem[a]
        elif kind == BIT:
            v = 1 if rem[a] == b else 0
        elif kind == BIT_SUM:
            v = 1 if rem[a] < b else 0
        elif kind == PRODUCT:
            v = inputs[state[a][b]] if rem[a] == b else 0
        elif kind == PROD_SUM:
            v = inputs[state[a][rem[a]]] if rem[a] < b else 0
        else:
            v = inputs[state[a + 1][b]]
        out.append(v % R)
    return out
