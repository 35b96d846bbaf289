"""The cases of tests/golden/vectors_g16.npz: one definition for the script that freezes them (tests/golden/make_vectors_g16.py), the CPU
test that holds g16_ref to the file and the GPU tests that hold the library to it.

A seeded generator of R1CS for which EVERY choice of the free variables extends to a satisfying assignment (a batch needs several
witnesses of one system).  Variables: the constant one, l - 1 public inputs, `free` private inputs, one output per "define"
constraint, and a last variable no row mentions (its query points are the point at infinity).  Constraint kinds:
  define   <A_i, z> * <B_i, z> = c z[out] + <C'_i, z> over earlier variables: fixes z[out]
  same     <A_i, z> * 1 = <A_i, z>: holds for every z; its rows take whatever shape is asked for -- one entry, 254 entries (a bit
           decomposition's row), SLICE + 8 entries (longer than the slice the kernel cuts rows into)
  empty    A_i and C_i have no entry
Rows are lists of (column, value) with distinct columns; matrices are lists of rows."""
import random

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SLICE = 32                    # csrc/groth16.hip kSlice: a row longer than this is cut

# name -> (domain n, l, n_constraints, free variables, define constraints); n_constraints + l = n ("full") or n / 2 + 1 ("half")
CASES = {
    "d8_full": (8, 2, 6, 4, 3),
    "d8_half": (8, 2, 3, 4, 2),
    "d64_full": (64, 3, 61, 256, 20),
    "d64_half": (64, 3, 30, 256, 12),
    "d1024_full": (1024, 7, 1017, 256, 24),
    "d1024_half": (1024, 7, 506, 256, 24),
}
BATCH = 3                     # frozen witnesses per case
BIG_BATCH = 129               # crosses the group of 128 (domain 8 only; its expected proofs are closed forms, not frozen)
REAL = (8192, 7, 8185, 4869)  # the reference key's shape: n, l, n_constraints, m


class System:
    def __init__(self, name, n, l, nc, m, A, B, C, defines, n_free):
        self.name, self.n, self.l, self.nc, self.m = name, n, l, nc, m
        self.A, self.B, self.C = A, B, C
        self.defines = defines           # (constraint, out variable, coefficient of z[out] in C)
        self.first_out = l + n_free      # variables below are chosen freely

    def matrices(self):
        return (self.A, self.B, self.C)


def _row(rng, hi, k):
    """k distinct columns below hi with non-zero values"""
    cols = sorted(rng.sample(range(hi), k))
    return [(c, rng.randrange(1, R)) for c in cols]


def system(name, n, l, nc, n_free, n_define, m=None):
    rng = random.Random(f"g16-system-{name}")
    assert nc + l <= n and n_define <= nc
    n_out = n_define
    m_min = l + n_free + n_out + 1
    m = m_min if m is None else m
    n_free += m - m_min
    first_out = l + n_free
    kinds = ["define"] * n_define + ["empty"] + ["same"] * (nc - n_define - 1)
    if nc - n_define - 1 < 0:
        kinds = ["define"] * n_define
    rng.shuffle(kinds)
    shapes = [1, 1, 2, 3]
    if first_out >= 254:
        shapes_once = [254, SLICE + 8, SLICE, SLICE + 1]
    else:
        shapes_once = [min(first_out, SLICE + 8)] if first_out > SLICE else []
    A, B, C, defines = [], [], [], []
    out = first_out
    for i, kind in enumerate(kinds):
        if kind == "empty":
            A.append([]); B.append(_row(rng, first_out, 2)); C.append([])
        elif kind == "same":
            k = shapes_once.pop() if shapes_once else rng.choice(shapes)
            row = _row(rng, out, min(k, out))
            A.append(row); B.append([(0, 1)]); C.append(list(row))
        else:
            A.append(_row(rng, out, min(out, rng.choice((1, 2, 3)))))
            B.append(_row(rng, out, min(out, rng.choice((1, 2)))))
            rest = _row(rng, out, rng.choice((0, 1, 2)))
            coef = rng.randrange(1, R)
            C.append(rest + [(out, coef)])
            defines.append((i, out, coef))
            out += 1
    assert out == m - 1 and not shapes_once
    return System(name, n, l, nc, m, A, B, C, defines, n_free)


def dot(row, z):
    return sum(v * z[c] for c, v in row) % R


def witness(sy, seed):
    """a satisfying assignment: the free variables from the seed, the outputs by forward evaluation, the unused last variable random"""
    rng = random.Random(f"g16-witness-{sy.name}-{seed}")
    z = [1] + [rng.randrange(R) for _ in range(sy.first_out - 1)] + [0] * (sy.m - sy.first_out)
    for i, out, coef in sy.defines:
        rest = dot(sy.C[i][:-1], z)
        z[out] = (dot(sy.A[i], z) * dot(sy.B[i], z) - rest) * pow(coef, R - 2, R) % R
    z[sy.m - 1] = rng.randrange(R)
    return z


def satisfied(sy, z):
    return all(dot(a, z) * dot(b, z) % R == dot(c, z) for a, b, c in zip(sy.A, sy.B, sy.C))


def blinds(name, seed):
    rng = random.Random(f"g16-blinds-{name}-{seed}")
    return rng.randrange(R), rng.randrange(R)


def trapdoor(name):
    rng = random.Random(f"g16-trapdoor-{name}")
    return tuple(rng.randrange(1, R) for _ in range(5))          # tau, alpha, beta, gamma, delta


def case_system(name):
    n, l, nc, n_free, n_define = CASES[name]
    return system(name, n, l, nc, n_free, n_define)


def real_system():
    """a stand-in of the reference circuit's SHAPE (its matrices exist only as Rust code): 500 define constraints, bit-decomposition
    sized rows among the rest"""
    n, l, nc, m = REAL
    return system("real-shape", n, l, nc, 256, 500, m=m)
