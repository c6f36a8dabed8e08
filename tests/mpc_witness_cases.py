"""Gate programs for the two-party witness sessions (include/bpgpu.h, bpgpu_mpc_witness_*) and what they must compute, in pure
Python: the cases, built on witness_cases.Program, and a model of the level-by-level protocol on integers -- the helper's own
dependency levels, and per level the planes of a_L and a_R of both parties, the masked values, their opening through the dealer and
the planes of a_O.  The reference of every test of the sessions: computed once per (case, batch) and left unchanged.  No GPU."""
import random

import mpc_dealer as md
import witness_cases as wc

pm = wc.pm
N = wc.N
MUL, INPUT, BIT = wc.MUL, wc.INPUT, wc.BIT
L, R, O, V, ONE = wc.L, wc.R, wc.O, wc.V, wc.ONE
EDGE = wc.EDGE
ROW_LENGTHS = wc.ROW_LENGTHS
RANGE_BITS = 8


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def range_inputs_case():
    """the range gadget on shares: a bit of a shared value is not a local function, so the bits come as INPUT pairs (1 - b, b); one
    MUL gate reads them all"""
    prog = wc.Program(1)
    for _ in range(RANGE_BITS):
        prog.input()
    prog.mul([(R, i, 1 << i) for i in range(RANGE_BITS)], [(L, i, 1) for i in range(RANGE_BITS)] + [(ONE, 0, N - 1)])
    pairs = lambda v: [(1 - ((v >> i) & 1), (v >> i) & 1) for i in range(RANGE_BITS)]    # noqa: E731
    provers = [([v], pairs(v), ()) for v in (0, (1 << RANGE_BITS) - 1, 1 << (RANGE_BITS - 1), 0xA5)]

    def gadget(cs, var, v, inputs):
        pm.range_proof_gadget(cs, pm.lc_var(var[0]), v[0], RANGE_BITS)
        left, right = {}, pm.lc_const(N - 1)
        for i in range(RANGE_BITS):
            left = pm.lc_add(left, {("R", i): 1 << i})
            right = pm.lc_add(right, {("L", i): 1})
        cs.multiply(left, right)
    # a value of 9 bits is no sum of the 8 bits given
    return wc.Case("range_inputs8", prog, provers, gadget, breaker=lambda v, inputs: ([1 << RANGE_BITS], inputs))


def mpc_wide_case():
    """a level of 300 MUL gates over the committed values and `One` terms with edge coefficients (more than a block of lanes), then a
    level of 5 gates that reads a_L / a_R / a_O of the first"""
    rnd = random.Random(3001)
    prog = wc.Program(4)
    for i in range(300):
        prog.mul([(V, i % 4, rnd.choice(EDGE)), (ONE, 0, rnd.choice(EDGE + (i,)))], [(V, (i + 1) % 4, 1), (ONE, 0, rnd.choice(EDGE))])
    for _ in range(5):
        prog.mul([(O, rnd.randrange(300), 1), (L, rnd.randrange(300), N - 1)], [(R, rnd.randrange(300), 1 << 251), (ONE, 0, 1)])
    prog.end_phase1()
    return wc.Case("mpc_wide", prog, [(wc._values(rnd, 4), (), ()) for _ in range(3)])


def mpc_edges_case(empty_phase1=False):
    """rows of every length on the lazy sums' fold boundaries and one above a lane's 64 terms, nchi = 3 in phase 2, INPUT gates in both
    phases, a last level of one gate; empty_phase1: the same second phase after no first one"""
    rnd = random.Random(2570 + empty_phase1)
    prog = wc.Program(3, nchi=3)
    if not empty_phase1:
        prog.input()
        for length in ROW_LENGTHS:
            i = prog.n
            prog.mul(wc._row(rnd, prog, i, length, False), wc._row(rnd, prog, i, ROW_LENGTHS[-1 - ROW_LENGTHS.index(length)], False))
        prog.mul([(V, 0, N - 1)] * 257, [(O, 1, N - 1)] * 33)       # the heaviest lazy sums: every product (n - 1) x (n - 1)
    prog.end_phase1()
    prog.input()
    for length in ROW_LENGTHS:
        i = prog.n
        prog.mul(wc._row(rnd, prog, i, length, True), wc._row(rnd, prog, i, 17, True))
    prog.mul([(V, 0, (None, None, None, N - 1))] * 257, [(R, prog.n - 1, (0, N - 1, None, None))] * 16)
    deep = prog.mul([(O, prog.n - 1, 1), (L, prog.n - 2, (1, None, 1, None))], [(ONE, 0, (None, 1, None, None))])
    prog.mul([(L, deep, 1), (R, deep, N - 1)], [(O, deep, (1, None, None, 1)), (ONE, 0, 1)])           # alone on the last level
    provers = []
    for chi in ((0, 0, 0), (1, 1, 1), (N - 1, N - 1, N - 1), tuple(rnd.randrange(N) for _ in range(3))):
        provers.append(([N - 1] + wc._values(rnd, 2), [tuple(wc._values(rnd, 2)) for _ in range(prog.ninp)], chi))
    return wc.Case("mpc_edges_p2" if empty_phase1 else "mpc_edges", prog, provers)


def dag_case(name, seed, n, n1, m, nchi, lengths, back=6):
    """a seeded random DAG over MUL, MUL, INPUT (witness_cases.generated_case without the BIT gates); back: how far below a term
    reaches, for depth"""
    rnd = random.Random(seed)
    prog = wc.Program(m, nchi)
    for i in range(n):
        if i == n1:
            prog.end_phase1()
        param = nchi > 0 and i >= n1
        if rnd.choice((MUL, MUL, INPUT)) == INPUT:
            prog.input()
        else:
            prog.mul(wc._row(rnd, prog, i, rnd.choice(lengths), param, back), wc._row(rnd, prog, i, rnd.choice(lengths), param, back))
    provers = []
    for _ in range(3):
        chi = tuple(rnd.choice(wc.CHIS + (rnd.randrange(N),)) for _ in range(nchi))
        provers.append((wc._values(rnd, m), [tuple(wc._values(rnd, 2)) for _ in range(prog.ninp)], chi))
    return wc.Case(name, prog, provers)


def gadget_cases():
    return [wc.example_case()] + [wc.shuffle_case(k) for k in (2, 3, 4, 9)] + [range_inputs_case()]


_cases = None


def cases():
    """every case, built once"""
    global _cases
    if _cases is None:
        _cases = gadget_cases() + [mpc_wide_case(), mpc_edges_case(), mpc_edges_case(True),
                                   dag_case("mpc_dag24", 2401, 24, 10, 2, 3, (0, 1, 3, 16, 17)),
                                   dag_case("mpc_dag70", 7001, 70, 40, 3, 1, (1, 2, 5, 9))]
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def gate_levels(prog):
    """level[i] of gate i inside its phase, from the definition: 0 for an INPUT gate or a gate whose rows read no multiplier of its own
    phase, else 1 + the largest level read"""
    level = []
    for i, (op, _, left, right) in enumerate(prog.gates):
        lo = 0 if i < prog.phase1 else prog.phase1
        reads = [idx for kind, idx, _ in left + right if kind <= O and idx >= lo]
        level.append(0 if op == INPUT or not reads else 1 + max(level[r] for r in reads))
    return level


def level_lists(prog, phase=0):
    """the rounds of a session of `phase`: per level its gates in ascending index, phase 1's levels first"""
    level = gate_levels(prog)
    out = []
    for ph, (lo, hi) in enumerate(((0, prog.phase1), (prog.phase1, prog.n))):
        if phase in (0, ph + 1):
            for l in range(max(level[lo:hi], default=-1) + 1):
                out.append([i for i in range(lo, hi) if level[i] == l])
    return out


def _row_on_plane(prog, row, chi, planes, v, k):
    """a row on plane k: a public coefficient scales every plane alike, a `One` term counts on the modifier plane only"""
    tot = 0
    for kind, idx, coeff in row:
        c = sum((part or 0) * (chi[j - 1] if j else 1) for j, part in enumerate(prog.parts(coeff)))
        tot += c * ((1 if k == 2 else 0) if kind == ONE else (planes[0], planes[1], planes[2], v)[kind][k][idx])
    return tot % N


class Model:
    """one batch of nb proofs of a case run as two parties on integers.  Operand bytes per party: v, inputs; chi (public); per level
    `rounds[l]` = dict(gates, triples[party] bytes, masked[party] bytes, opened bytes); planes[party] = (a_L, a_R, a_O) bytes;
    witness[p] = the opened (a_L, a_R, a_O); zero_d: (level, proof, slot) whose opened d is zero by the choice of its triple"""

    def __init__(self, case_, nb, seed=11, which=None):
        prog = case_.prog
        self.case, self.nb, self.dealer = case_, nb, md.Dealer(seed)
        d = self.dealer
        provers = [case_.prover(p) if which is None else which(p) for p in range(nb)]
        self.provers = provers
        n, ninp = prog.n, prog.ninp
        v_sh = [d.share_vec(pr[0]) for pr in provers]                                     # [proof][party][plane][i]
        l_sh = [d.share_vec([pair[0] for pair in pr[1]]) for pr in provers]
        r_sh = [d.share_vec([pair[1] for pair in pr[1]]) for pr in provers]
        self.v = [md.pack([[v_sh[p][q][k] for k in range(3)] for p in range(nb)]) or None for q in range(2)]
        self.inputs = [md.pack([[[x for j in range(ninp) for x in (l_sh[p][q][k][j], r_sh[p][q][k][j])] for k in range(3)]
                                for p in range(nb)]) or None for q in range(2)]
        self.chi = b"".join(md.le(x) for pr in provers for x in pr[2]) or None
        # planes[proof][party][a_L, a_R, a_O][plane][gate]
        pl = [[[[[0] * n for _ in range(3)] for _ in range(3)] for _ in range(2)] for _ in range(nb)]
        pair_of, pairs = {}, 0
        for i, g in enumerate(prog.gates):
            if g[0] == INPUT:
                pair_of[i] = pairs
                pairs += 1
        self.rounds, self.zero_d = [], None
        for lvl, gates in enumerate(level_lists(prog)):
            G = len(gates)
            trip = []
            for p in range(nb):
                chi = provers[p][2]
                for q in range(2):
                    for k in range(3):
                        for i in gates:
                            op, _, left, right = prog.gates[i]
                            if op == INPUT:
                                a, b = l_sh[p][q][k][pair_of[i]], r_sh[p][q][k][pair_of[i]]
                            else:
                                a = _row_on_plane(prog, left, chi, pl[p][q], v_sh[p][q], k)
                                b = _row_on_plane(prog, right, chi, pl[p][q], v_sh[p][q], k)
                            pl[p][q][0][k][i], pl[p][q][1][k][i] = a, b
                t = d.triples(G)                                                          # [party][x, y, z][plane][slot]
                if self.zero_d is None:
                    # one triple of the case chosen with x = a_L of its gate: the opened d is zero
                    i = gates[0]
                    x = (pl[p][0][0][0][i] + pl[p][1][0][0][i] + pl[p][0][0][2][i]) % N
                    y = d.rnd.randrange(N)
                    for which_t, val in enumerate((x, y, x * y % N)):
                        sh = d.share(val, modifier=False)
                        for q in range(2):
                            for k in range(3):
                                t[q][which_t][k][0] = sh[q][k]
                    self.zero_d = (lvl, p, 0)
                trip.append(t)
            masked = [[[[[(pl[p][q][de][k][i] - trip[p][q][de][k][s]) % N for s, i in enumerate(gates)] for k in range(3)] for de in range(2)]
                       for p in range(nb)] for q in range(2)]
            opened = [[[d.open_sc("%s %d[%d][%d]" % ("de"[de], lvl, p, s), [tuple(masked[q][p][de][k][s] for k in range(3)) for q in range(2)])
                        for s in range(G)] for de in range(2)] for p in range(nb)]
            for p in range(nb):
                for q in range(2):
                    for k in range(3):
                        for s, i in enumerate(gates):
                            dd, ee = opened[p][0][s], opened[p][1][s]
                            x, y, z = (trip[p][q][w][k][s] for w in range(3))
                            pl[p][q][2][k][i] = (z + dd * y + ee * x + (dd * ee if k == 2 else 0)) % N
            self.rounds.append(dict(gates=gates, triples=[md.pack([trip[p][q] for p in range(nb)]) for q in range(2)],
                                    masked=[md.pack(masked[q]) for q in range(2)], opened=md.pack(opened), opened_ints=opened,
                                    triples_ints=trip, masked_ints=masked))      # ints: [proof][party][x, y, z][plane][slot], [party][proof][d, e][plane][slot]
        assert self.zero_d is None or self.rounds[self.zero_d[0]]["opened_ints"][self.zero_d[1]][0][0] == 0
        self.ints = pl
        self.planes = [tuple(md.pack([[pl[p][q][w][k] for k in range(3)] for p in range(nb)]) for w in range(3)) for q in range(2)]
        self.witness = [tuple([d.open_sc("%s[%d][%d]" % ("LRO"[w], p, i), [tuple(pl[p][q][w][k][i] for k in range(3)) for q in range(2)])
                               for i in range(n)] for w in range(3)) for p in range(nb)]

    def opened_operands(self):
        """(v, inputs, chi) of the batch as bpgpu_r1cs_witness_synthesize takes them: the opened values"""
        return self.case.operands(self.nb, which=lambda p: self.provers[p])


_models = {}


def model(case_, nb):
    """the model of (case, nb), computed once"""
    key = (case_.name, nb)
    if key not in _models:
        _models[key] = Model(case_, nb)
    return _models[key]


def open_planes(dealer, name, planes, nb, count):
    """planes[party]: nb x 3 x count ark bytes -> [proof][i] opened through the dealer (MAC and modifier checks recorded under name)"""
    vals = [[md.unmont(b) for b in md.cut(pl, 32)] for pl in planes]
    return [[dealer.open_sc("%s[%d][%d]" % (name, p, i), [tuple(vals[q][(p * 3 + k) * count + i] for k in range(3)) for q in range(2)])
             for i in range(count)] for p in range(nb)]
