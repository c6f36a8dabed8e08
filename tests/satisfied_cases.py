"""Inputs and the model of bpgpu_r1cs_constraints_satisfied / bpgpu_mpc_constraints_eval (include/bpgpu.h): Python integers only.
e[p][r] = sum over the row's terms of coeff * value mod n, over the test's own list of rows; the gate identity the same way.
Circuits come from tests/circuit_gen.py (their witnesses satisfy them for every chi; broken() moves one constant by one) or are
hand-built rows, which go through mpc_dealer.circuit_rows so that repeated variables and zero coefficients stay separate terms.
No GPU needed."""
import os
import random
import re

import circuit_gen as cg
import lazy_sum_cases as lz
import mpc_dealer as md

pm = cg.pm
N = pm.N
ONE = pm.ONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lane_max():
    """the route threshold T of csrc/k_rows.hip: a row of up to T terms is a lane's, a longer one a wave's"""
    src = open(os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", "k_rows.hip")).read()
    return int(re.search(r"#define ROWS_LANE_MAX (\d+)", src).group(1))


def row_lengths(T):
    return sorted({0, 1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 257, T - 1, T, T + 1})


class Witness:
    """one prover's operands: a_L, a_R, a_O (n each) and the committed values v (m)"""

    def __init__(self, a_L, a_R, v, a_O=None):
        self.a_L, self.a_R, self.v = list(a_L), list(a_R), list(v)
        self.a_O = [x * y % N for x, y in zip(a_L, a_R)] if a_O is None else list(a_O)

    def value(self, var):
        return 1 if var == ONE else {"L": self.a_L, "R": self.a_R, "O": self.a_O, "V": self.v}[var[0]][var[1]]

    def copy(self):
        return Witness(self.a_L, self.a_R, self.v, self.a_O)


def witness_of(circ):
    return Witness(circ.a_L, circ.a_R, circ.v)


def residuals(rows, wit, chi=()):
    """the model: e[r] for one prover"""
    return [sum(cg.coeff_at(c, chi) * wit.value(var) for var, c in row) % N for row in rows]


def first_bad(values):
    return next((i for i, e in enumerate(values) if e), -1)


def first_bad_gate(wit):
    return first_bad([(x * y - z) % N for x, y, z in zip(wit.a_L, wit.a_R, wit.a_O)])


def expect(rows, wits, chis=None):
    """-> (ok, first_bad_row, first_bad_gate, residuals) of a batch, as the call returns them"""
    es = [residuals(rows, w, chis[p] if chis else ()) for p, w in enumerate(wits)]
    row, gate = [first_bad(e) for e in es], [first_bad_gate(w) for w in wits]
    return [int(r < 0 and g < 0) for r, g in zip(row, gate)], row, gate, es


def planes(wits):
    """the ark-form operands of a batch: a_L, a_R, a_O, v (None where the circuit has none)"""
    cat = lambda key: b"".join(md.mont(x) for w in wits for x in getattr(w, key)) or None      # noqa: E731
    return cat("a_L"), cat("a_R"), cat("a_O"), cat("v")


def chi_bytes(chis):
    return b"".join(md.le(x) for chi in chis for x in chi) if chis and chis[0] else None


def res_bytes(es):
    return b"".join(md.le(e) for row in es for e in row)


def csr(rows, nchi=0):
    """(row_ptr, kind, idx, coeff) for circuit_create (nchi == 0) or circuit_create_param"""
    return md.circuit_rows(rows, nchi=nchi if nchi else None)[:4]


def length_rows(T, n=6, m=2, seed=11):
    """Hand-built rows of every length of row_lengths(T) in ONE circuit -- so both routes run in one launch -- with coefficients and
    values at 0, 1 and n - 1 beside random ones, then: a row of 257 of the heaviest products (coefficient x value = -2^-261, each lazily
    n - 1: tests/lazy_sum_cases.py), the all-(n - 1) x (n - 1) row of 257 terms (each lazily the 251-bit 2^261 mod n), a row of
    explicit zero terms, a row of one variable repeated, rows of `One` terms only (a non-zero constant alone, a zero constant alone,
    two constants that cancel).  -> (rows, witness); the rows are NOT satisfied: the model's residuals are the expectation."""
    rnd = random.Random(seed)
    a_L = [0, 1, N - 1] + [rnd.randrange(N) for _ in range(n - 3)]
    a_R = [N - 1, N - 1, N - 1] + [rnd.randrange(N) for _ in range(n - 3)]
    wit = Witness(a_L, a_R, [N - 1] + [rnd.randrange(N) for _ in range(m - 1)])
    variables = [(k, i) for k in "LRO" for i in range(n)] + [("V", i) for i in range(m)] + [ONE]
    rows = []
    for length in row_lengths(T):
        rows.append([(rnd.choice(variables), rnd.choice((0, 1, N - 1, rnd.randrange(N)))) for _ in range(length)])
    rows.append([(("L", 3), lz.C * pow(a_L[3], -1, N) % N)] * 257)
    rows.append([(("L", 2), N - 1)] * 257)
    rows.append([(rnd.choice(variables), 0) for _ in range(T + 3)])
    rows.append([(("R", 3), rnd.randrange(N)) for _ in range(40)])
    rows += [[(ONE, 5)], [(ONE, 0)], [(ONE, 3), (ONE, N - 3)], [(ONE, 1)] * (T + 2)]
    return rows, wit


def with_constant(rows, *bad_rows):
    """the rows with an extra `One` term of 1 in each of bad_rows: a satisfied row stops being one"""
    return [list(row) + ([(ONE, 1)] if r in bad_rows else []) for r, row in enumerate(rows)]


def chi_fault(circ):
    """a parametric circuit's rows with one constant's chi_1 part moved by one: satisfied at chi = 0 only -> (rows, the row)"""
    rows = [list(row) for row in circ.rows]
    for r in range(circ.q1, circ.q):
        for t, (var, c) in enumerate(rows[r]):
            if var == ONE and isinstance(c, tuple):
                rows[r][t] = (var, (c[0], ((c[1] or 0) + 1) % N) + c[2:])
                return rows, r
    raise ValueError("no second-phase constant")


# (q, nb, n, m): every edge of the grid -- q in {1, 255, 256, 257}, nb in {1, 3, 65}, n in {0, 1, 64, 65}, m in {0, 2}
GRID = [(q, nb, n, m) for q in (1, 255, 256, 257) for nb, n, m in ((1, 0, 2), (3, 1, 0), (65, 64, 2), (3, 65, 0))]
# generated parametric circuits: (seed, n1, n2, m, q, nchi, profile)
PARAM = [(41, 2, 2, 1, 8, 1, "sparse"), (42, 3, 2, 2, 10, 2, "dups"), (43, 2, 3, 1, 12, 8, "dense")]


def grid_circuit(q, n, m):
    return cg.Circuit(7000 + q + 3 * n + m, n, 0, m, q, 0, "sparse")
