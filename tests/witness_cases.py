"""Gate programs for bpgpu_witness (include/bpgpu.h) and what they must compute, in pure Python on the model (oracle/pymodel.py): a
builder per program, a reference evaluator on integers, and for every gadget case the witness the model's Prover assigns when the
same gadget runs on it.  The reference of every test of the witness synthesis: computed once per case and left unchanged.  No GPU."""
import random

import circuit_gen as cg
import mpc_dealer as md

pm = cg.pm
N = pm.N
le, mont = md.le, md.mont
MUL, INPUT, BIT = 0, 1, 2
L, R, O, V, ONE = 0, 1, 2, 3, 4                       # term kinds of the CSR
EDGE = (0, 1, N - 1, (N + 1) // 2, 1 << 251)          # coefficients and values at the edges of the field
SHUFFLE_LABEL = b"shuffle challenge"
LANE_MAX = 64                                         # rows_lane_max() of csrc/k_rows.hip: a longer row is a wave's


class Program:
    """n gates in order, the first n1 in phase 1.  A row is a list of terms (kind, idx, coeff); coeff an integer (the constant part)
    or a tuple (c0, c1, .., c_nchi) standing for c0 + sum_j chi_j c_j, None parts stored nowhere, explicit zeros kept as terms."""

    def __init__(self, m, nchi=0):
        self.m, self.nchi, self.gates, self.n1 = m, nchi, [], None

    def _add(self, op, arg, left, right):
        self.gates.append((op, arg, list(left), list(right)))
        return len(self.gates) - 1

    def mul(self, left, right):
        return self._add(MUL, 0, left, right)

    def input(self):
        return self._add(INPUT, 0, (), ())

    def bit(self, left, bit):
        return self._add(BIT, bit, left, ())

    def end_phase1(self):
        self.n1 = len(self.gates)

    @property
    def n(self):
        return len(self.gates)

    @property
    def phase1(self):
        return self.n if self.n1 is None else self.n1

    @property
    def ninp(self):
        return sum(1 for g in self.gates if g[0] == INPUT)

    def ops(self):
        return [g[0] for g in self.gates]

    def args(self):
        return [g[1] for g in self.gates]

    def parts(self, coeff):
        return tuple(coeff) if isinstance(coeff, tuple) else (coeff,) + (None,) * self.nchi

    def csr(self):
        """(row_ptr, kind, idx, coeff) of bpgpu_witness_create: (1 + nchi) * 2 n stored rows, block j the chi_j parts"""
        rp, kd, ix, cf = [0], [], [], []
        for j in range(1 + self.nchi):
            for _, _, left, right in self.gates:
                for row in (left, right):
                    for kind, idx, coeff in row:
                        c = self.parts(coeff)[j]
                        if c is not None:
                            kd.append(kind)
                            ix.append(idx)
                            cf.append(le(c))
                    rp.append(len(kd))
        return rp, kd, ix, b"".join(cf)

    def create_args(self):
        """the arguments of BpGpu.witness_create"""
        return (self.n, self.phase1, self.m, self.nchi, self.ops(), self.args()) + self.csr()

    def plan_args(self):
        rp, kd, ix, _ = self.csr()
        return self.n, self.phase1, self.nchi, self.ops(), rp, kd, ix

    def row_len(self, row):
        return sum(1 for _, _, c in row for part in self.parts(c) if part is not None)

    def levels(self):
        """the helper's own dependency levels -> (levels of phase 1, of phase 2, widest level, long rows)"""
        level, width = [], ({}, {})
        for i, (op, _, left, right) in enumerate(self.gates):
            lo = 0 if i < self.phase1 else self.phase1
            reads = [idx for kind, idx, _ in left + right if kind <= O and idx >= lo]
            level.append(0 if op == INPUT or not reads else 1 + max(level[r] for r in reads))
            w = width[i >= self.phase1]
            w[level[i]] = w.get(level[i], 0) + 1
        long_rows = sum(1 for _, _, left, right in self.gates for row in (left, right) if self.row_len(row) > LANE_MAX)
        return len(width[0]), len(width[1]), max(list(width[0].values()) + list(width[1].values()) + [0]), long_rows

    def evaluate(self, v, inputs=(), chi=(), phase=0, planes=None):
        """the witness on integers -> (a_L, a_R, a_O); phase 2 continues the planes given"""
        aL, aR, aO = ([0] * self.n for _ in range(3)) if planes is None else (list(p) for p in planes)
        lo, hi = (0 if phase != 2 else self.phase1), (self.phase1 if phase == 1 else self.n)
        pair = sum(1 for g in self.gates[:lo] if g[0] == INPUT)

        def ev(row):
            tot = 0
            for kind, idx, coeff in row:
                c = sum((part or 0) * (chi[j - 1] if j else 1) for j, part in enumerate(self.parts(coeff)))
                tot += c * (1 if kind == ONE else (aL, aR, aO, v)[kind][idx])
            return tot % N
        for i in range(lo, hi):
            op, arg, left, right = self.gates[i]
            if op == INPUT:
                aL[i], aR[i] = inputs[pair][0] % N, inputs[pair][1] % N
                pair += 1
            elif op == BIT:
                b = (ev(left) >> arg) & 1
                aL[i], aR[i] = 1 - b, b
            else:
                aL[i], aR[i] = ev(left), ev(right)
            aO[i] = aL[i] * aR[i] % N
        return aL, aR, aO


class Case:
    """a program and its provers: (v, inputs, chi) each; gadget: a function (model prover, committed variables, v) -> None that runs
    the reference's gadget, for the cases that have one"""

    def __init__(self, name, prog, provers, gadget=None, breaker=None):
        self.name, self.prog, self.provers, self.gadget, self.breaker = name, prog, provers, gadget, breaker
        self._want = {}

    def prover(self, p):
        return self.provers[p % len(self.provers)]

    def want(self, p):
        """the helper's witness of prover p (computed once)"""
        p %= len(self.provers)
        if p not in self._want:
            v, inputs, chi = self.provers[p]
            self._want[p] = self.prog.evaluate(v, inputs, chi)
        return self._want[p]

    def model(self, p, transcript_label=b"witness case"):
        """the model's Prover after the gadget ran on prover p's values, its second phase on the case's challenge -> the prover"""
        v, inputs, chi = self.prover(p)
        pv = pm.Prover(pm.PedersenGens(), pm.Transcript(transcript_label))
        pv.v, pv.v_blinding = [x % N for x in v], [0] * len(v)        # (the commitments themselves are not needed here)
        self.gadget(pv, [("V", i) for i in range(len(v))], v, inputs)
        if chi:
            pv.challenge_scalar = lambda label: chi[0]
        pv._create_randomized_constraints()
        return pv

    def operands(self, nb, which=None):
        """(v, inputs, chi) of a batch of nb provers as the ABI takes them: ark, ark, canonical LE (None where the program has none)"""
        ps = [self.prover(p) if which is None else which(p) for p in range(nb)]
        v = b"".join(mont(x) for pr in ps for x in pr[0]) or None
        inputs = b"".join(mont(x) for pr in ps for pair in pr[1] for x in pair) or None
        chi = b"".join(le(x) for pr in ps for x in pr[2]) or None
        return v, inputs, chi

    def planes(self, nb, lo=0, hi=None):
        """the expected planes of a batch, ark form; lo, hi: a slice of every prover's multipliers"""
        hi = self.prog.n if hi is None else hi
        return tuple(b"".join(mont(x) for p in range(nb) for x in self.want(p)[k][lo:hi]) for k in range(3))


# ---- the reference's gadgets as programs -------------------------------------------------------------------------------------------
def range_case(bits, m):
    prog = Program(m)
    for j in range(m):
        for i in range(bits):
            prog.bit([(V, j, 1)], i)
    values = (0, (1 << bits) - 1, 1 << (bits - 1))
    provers = [([values[(p + j) % 3] for j in range(m)], (), ()) for p in range(3)]

    def gadget(cs, var, v, inputs):
        for j in range(m):
            pm.range_proof_gadget(cs, pm.lc_var(var[j]), v[j], bits)
    # a value of `bits + 1` bits is no sum of its low bits
    return Case("range%dx%d" % (bits, m), prog, provers, gadget, breaker=lambda v, inputs: ([1 << bits] + list(v[1:]), inputs))


def _example_rows(base):
    return [(V, base, 1), (V, base + 1, 1)], [(V, base + 2, 1), (V, base + 3, 1)]


def _example_values(rnd):
    a1, a2, b1, b2, c1 = (rnd.randrange(N) for _ in range(5))
    return [a1, a2, b1, b2, c1, ((a1 + a2) * (b1 + b2) - c1) % N]


def example_case():
    prog = Program(6)
    prog.mul(*_example_rows(0))
    rnd = random.Random(31)
    provers = [(_example_values(rnd), (), ()) for _ in range(3)]

    def gadget(cs, var, v, inputs):
        pm.example_gadget(cs, *(pm.lc_var(x) for x in var))
    return Case("example", prog, provers, gadget, breaker=lambda v, inputs: (list(v[:4]) + [(v[4] + 1) % N, v[5]], inputs))


def _shuffle_gates(prog, k, base):
    """tests/r1cs.rs:36-61 over the committed values base .. base + 2 k: two chains of multiply(prev_out, x_i - z)"""
    mz = (ONE, 0, (None, N - 1))
    for side in (base, base + k):
        last = prog.mul([(V, side + k - 1, 1), mz], [(V, side + k - 2, 1), mz])
        for i in range(k - 3, -1, -1):
            last = prog.mul([(O, last, 1)], [(V, side + i, 1), mz])


def _shuffle_values(rnd, k):
    xs = [rnd.getrandbits(40) for _ in range(k)]
    ys = list(xs)
    rnd.shuffle(ys)
    return xs + ys


CHIS = (0, 1, N - 1)


def shuffle_case(k):
    prog = Program(2 * k, nchi=1)
    prog.end_phase1()
    _shuffle_gates(prog, k, 0)
    rnd = random.Random(50 + k)
    provers = [(_shuffle_values(rnd, k), (), (chi,)) for chi in CHIS + (rnd.randrange(N), rnd.randrange(N))]

    def gadget(cs, var, v, inputs):
        pm.shuffle_gadget(cs, var[:k], var[k:])
    return Case("shuffle%d" % k, prog, provers, gadget, breaker=lambda v, inputs: ([(v[0] + 1) % N] + list(v[1:]), inputs))


COMPOSITE_BITS, COMPOSITE_K = 8, 3


def composite_case():
    """phase 1: the range gates of V_0 (BIT), example_gadget over V_1..V_6 (MUL) and two allocate_multiplier calls (INPUT); phase 2: a
    shuffle of V_7..V_12"""
    k = COMPOSITE_K
    prog = Program(7 + 2 * k, nchi=1)
    for i in range(COMPOSITE_BITS):
        prog.bit([(V, 0, 1)], i)
    prog.mul(*_example_rows(1))
    prog.input()
    prog.input()
    prog.end_phase1()
    _shuffle_gates(prog, k, 7)
    rnd = random.Random(77)
    provers = []
    for chi in CHIS + (rnd.randrange(N), rnd.randrange(N)):
        v = [rnd.getrandbits(COMPOSITE_BITS)] + _example_values(rnd) + _shuffle_values(rnd, k)
        provers.append((v, [(rnd.randrange(N), rnd.randrange(N)), (N - 1, rnd.choice(EDGE))], (chi,)))

    def gadget(cs, var, v, inputs):
        pm.range_proof_gadget(cs, pm.lc_var(var[0]), v[0], COMPOSITE_BITS)
        pm.example_gadget(cs, *(pm.lc_var(x) for x in var[1:7]))
        for pair in inputs:
            cs.allocate_multiplier(pair)
        pm.shuffle_gadget(cs, var[7:7 + k], var[7 + k:])
    return Case("composite", prog, provers, gadget, breaker=lambda v, inputs: (list(v[:7]) + [(v[7] + 1) % N] + list(v[8:]), inputs))


def circuit_csr(case, p=0):
    """the parametric circuit (q, nchi, row_ptr, kind, idx, coeff) of a gadget case from the model's constraints: a `One` term of a
    second-phase constraint is the shuffle's -z, stored as -1 in the chi block"""
    pv = case.model(p)
    return circuit_from(pv.constraints, len(pm_constraints_phase1(case, p)), case.prover(p)[2], case.prog.nchi)


def circuit_from(constraints, q1, chi, nchi):
    """(q, nchi, row_ptr, kind, idx, coeff) of a model prover's constraints, the first q1 of them from phase 1, the others evaluated on
    the gadget challenge chi[0]"""
    rows = []
    for r, lc in enumerate(constraints):
        row = []
        for var, c in lc.items():
            if chi and r >= q1 and var == pm.ONE:
                assert c == (-chi[0]) % N
                row.append((var, (None, N - 1)))
            else:
                row.append((var, c))
        rows.append(row)
    rp, kd, ix, cf, _ = md.circuit_rows(rows, nchi=nchi)
    return len(rows), nchi, rp, kd, ix, cf


def pm_constraints_phase1(case, p):
    v, inputs, _ = case.prover(p)
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"witness case"))
    pv.v, pv.v_blinding = [x % N for x in v], [0] * len(v)
    case.gadget(pv, [("V", i) for i in range(len(v))], v, inputs)
    return pv.constraints


# ---- generated programs: seeded random DAGs over the three ops ---------------------------------------------------------------------
def _coeff(rnd, nchi, param):
    c0 = rnd.choice(EDGE + (rnd.randrange(N),))
    if not param:
        return c0
    return (rnd.choice((None, c0)),) + tuple(rnd.choice((None, 0, rnd.choice(EDGE), rnd.randrange(N))) for _ in range(nchi))


def _row(rnd, prog, i, length, param, back=None):
    """`length` stored terms over the committed values, the constant and the gates below i (back: how far below)"""
    row, left = [], length
    while left > 0:
        kinds = [V, ONE] + ([L, R, O] if i else [])
        kind = rnd.choice(kinds)
        idx = 0 if kind == ONE else (rnd.randrange(prog.m) if kind == V else rnd.randrange(max(0, i - back) if back else 0, i))
        coeff = _coeff(rnd, prog.nchi, param)
        stored = prog.row_len([(kind, idx, coeff)])
        if stored == 0 or stored > left:
            coeff = rnd.choice(EDGE)
            stored = 1
        row.append((kind, idx, coeff))
        left -= stored
    return row


def _values(rnd, count):
    return [rnd.choice(EDGE + (rnd.randrange(N),)) for _ in range(count)]


def generated_case(name, seed, n, n1, m, nchi, lengths, nprovers=3, back=None):
    """a random DAG: gate i draws its op and the lengths of its rows; gates from n1 on may carry chi parts"""
    rnd = random.Random(seed)
    prog = Program(m, nchi)
    for i in range(n):
        if i == n1:
            prog.end_phase1()
        param = nchi > 0 and i >= n1
        op = rnd.choice((MUL, MUL, MUL, INPUT, BIT))
        if op == INPUT:
            prog.input()
        elif op == BIT:
            prog.bit(_row(rnd, prog, i, rnd.choice(lengths), param, back), rnd.choice((0, 1, 63, 200, 251)))
        else:
            prog.mul(_row(rnd, prog, i, rnd.choice(lengths), param, back), _row(rnd, prog, i, rnd.choice(lengths), param, back))
    if n1 >= n:
        prog.end_phase1()
    provers = []
    for p in range(nprovers):
        chi = tuple(rnd.choice(CHIS + (rnd.randrange(N),)) for _ in range(nchi))
        provers.append((_values(rnd, m), [tuple(_values(rnd, 2)) for _ in range(prog.ninp)], chi))
    return Case(name, prog, provers)


def wide_case():
    """a level of 300 gates over the committed values alone (wider than a block: the strided loop), then a second level that reads it"""
    rnd = random.Random(300)
    prog = Program(4)
    for i in range(300):
        if i % 7 == 3:
            prog.bit([(V, i % 4, 1), (ONE, 0, rnd.choice(EDGE))], rnd.choice((0, 63, 251)))
        else:
            prog.mul([(V, i % 4, rnd.choice(EDGE)), (ONE, 0, i)], [(V, (i + 1) % 4, 1)])
    for i in range(5):
        prog.mul([(O, rnd.randrange(300), 1), (L, rnd.randrange(300), N - 1)], [(R, rnd.randrange(300), 1 << 251)])
    prog.end_phase1()
    return Case("wide300", prog, [(_values(rnd, 4), (), ()) for _ in range(3)])


ROW_LENGTHS = (0, 1, 15, 16, 17, 33, 257)


def edges_case():
    """rows of every length on the lazy sums' fold boundaries and one above rows_lane_max(), nchi = 3 in phase 2, and the bit
    extraction on bits 0, 63 and 251 of n - 1 (read through a committed value, through the constant and through a product)"""
    rnd = random.Random(257)
    prog = Program(3, nchi=3)
    for b in (0, 63, 251):
        prog.bit([(V, 0, 1)], b)                  # v_0 = n - 1
        prog.bit([(ONE, 0, N - 1)], b)
    prog.mul([(V, 0, 1)], [(ONE, 0, 1)])          # gate 6: a_O = n - 1
    for b in (0, 63, 251):
        prog.bit([(O, 6, 1)], b)
    for length in ROW_LENGTHS:
        i = prog.n
        prog.mul(_row(rnd, prog, i, length, False), _row(rnd, prog, i, ROW_LENGTHS[-1 - ROW_LENGTHS.index(length)], False))
    # the heaviest lazy sums: every product (n - 1) x (n - 1)
    prog.mul([(V, 0, N - 1)] * 257, [(O, 6, N - 1)] * 33)
    prog.end_phase1()
    for length in ROW_LENGTHS:
        i = prog.n
        prog.mul(_row(rnd, prog, i, length, True), _row(rnd, prog, i, 17, True))
        prog.bit(_row(rnd, prog, i + 1, length, True), rnd.choice((0, 63, 251)))
    prog.mul([(V, 0, (None, None, None, N - 1))] * 257, [(R, 6, (0, N - 1, None, None))] * 16)
    provers = []
    for chi in ((0, 0, 0), (1, 1, 1), (N - 1, N - 1, N - 1), tuple(rnd.randrange(N) for _ in range(3))):
        provers.append(([N - 1] + _values(rnd, 2), (), chi))
    return Case("edges", prog, provers)


def gadget_cases():
    return ([range_case(bits, m) for bits in (8, 64) for m in (1, 3)] + [example_case()] + [shuffle_case(k) for k in (2, 3, 4, 9)] +
            [composite_case()])


def generated_cases():
    return [generated_case("gen1", 1, 1, 1, 1, 0, (0, 1, 2)),
            generated_case("gen70dense", 70, 70, 40, 3, 1, (1, 2, 5, 9), back=6),
            generated_case("gen24chi3", 24, 24, 10, 2, 3, (0, 1, 3, 16, 17)),
            wide_case(), edges_case()]


_cases = None


def cases():
    """every case, built once"""
    global _cases
    if _cases is None:
        _cases = gadget_cases() + generated_cases()
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)
