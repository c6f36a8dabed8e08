"""Gate programs with BPGPU_GATE_INV gates (include/bpgpu.h: a_L = eval(left), a_R = a_L^-1 or 0, a_O = a_L a_R) on the Program of
tests/witness_cases.py: the op, its evaluation on Python integers (pow(x, N - 2, N), 0 for 0), programs that put a level's INV gates
on every boundary of the batched inversion of csrc/k_witness.hip (256 threads, thread t owns the gates t, t + 256, ..), and the
is-zero gadget run on the model prover.  The reference of every test: computed once per case and left unchanged.  No GPU."""
import random

import witness_cases as wc

pm = wc.pm
N = wc.N
L, R, O, V, ONE = wc.L, wc.R, wc.O, wc.V, wc.ONE
INV = 4                                               # BPGPU_GATE_INV; 3 is no op
LEVEL_SIZES = (1, 3, 255, 256, 257, 513)              # runs of 1, 2 and 3 gates per thread, and ragged ones
LABEL = wc.SHUFFLE_LABEL


def inv_or_zero(x):
    return pow(x % N, N - 2, N)


class Program(wc.Program):
    def inv(self, left):
        return self._add(INV, 0, left, ())

    def evaluate(self, v, inputs=(), chi=(), phase=0, planes=None):
        """the witness on integers, op 4 included -> (a_L, a_R, a_O); phase 2 continues the planes given"""
        aL, aR, aO = ([0] * self.n for _ in range(3)) if planes is None else (list(p) for p in planes)
        lo, hi = (0 if phase != 2 else self.phase1), (self.phase1 if phase == 1 else self.n)
        pair = sum(1 for g in self.gates[:lo] if g[0] == wc.INPUT)

        def ev(row):
            tot = 0
            for kind, idx, coeff in row:
                c = sum((part or 0) * (chi[j - 1] if j else 1) for j, part in enumerate(self.parts(coeff)))
                tot += c * (1 if kind == ONE else (aL, aR, aO, v)[kind][idx])
            return tot % N
        for i in range(lo, hi):
            op, arg, left, right = self.gates[i]
            if op == wc.INPUT:
                aL[i], aR[i] = inputs[pair][0] % N, inputs[pair][1] % N
                pair += 1
            elif op == wc.BIT:
                b = (ev(left) >> arg) & 1
                aL[i], aR[i] = 1 - b, b
            elif op == INV:
                aL[i] = ev(left)
                aR[i] = inv_or_zero(aL[i])
            else:
                aL[i], aR[i] = ev(left), ev(right)
            aO[i] = aL[i] * aR[i] % N
        return aL, aR, aO


# ---- levels of INV gates over the committed values: zeros wherever a thread's run can meet them -------------------------------------
def _nonzero(rnd):
    return rnd.choice(wc.EDGE[1:] + (rnd.randrange(1, N),))


def level_case(size):
    """one level of `size` INV gates, gate i = inv(v_i), then a MUL level that reads a_R and a_O of the first, the middle and the
    last; provers: no zero, a zero first, last, at each position of thread 0's run alone, at all of them, every second gate, all"""
    rnd = random.Random(4000 + size)
    prog = Program(size)
    for i in range(size):
        prog.inv([(V, i, 1)])
    for i in sorted({0, size // 2, size - 1}):
        prog.mul([(R, i, 1), (O, i, N - 1)], [(L, i, 1), (ONE, 0, 1)])
    prog.end_phase1()
    run0 = list(range(0, size, 256))
    zero_sets = [[], [0], [size - 1]] + [[i] for i in run0] + [run0, list(range(0, size, 2)), list(range(size))]
    provers = []
    for zeros in zero_sets:
        v = [_nonzero(rnd) for _ in range(size)]
        for i in zeros:
            v[i] = 0
        provers.append((v, (), ()))
    return wc.Case("inv_level%d" % size, prog, provers)


def edge_values_case():
    """the values 0, 1, N - 1, (N + 1) / 2, 2^251 read straight, through a coefficient, and as sums that wrap to zero"""
    prog = Program(len(wc.EDGE))
    for j in range(len(wc.EDGE)):
        prog.inv([(V, j, 1)])
        prog.inv([(V, j, N - 1)])
        prog.inv([(V, j, 1), (V, j, N - 1)])                       # x - x
        prog.inv([(V, j, 1), (ONE, 0, 1)])                         # x + 1: zero for N - 1
        prog.inv([(V, j, 2), (ONE, 0, N - 1)])                     # 2 x - 1: zero for (N + 1) / 2
    prog.end_phase1()
    return wc.Case("inv_edges", prog, [(list(wc.EDGE), (), ()), (list(reversed(wc.EDGE)), (), ())])


def long_row_case():
    """INV gates with a row of 257 terms (a wave's in the block form: one inversion each, by lane 0) beside short ones on one level:
    the heaviest lazy sum, a long sum that is zero, a long sum that wraps"""
    prog = Program(2)
    prog.inv([(V, 0, N - 1)] * 257)
    prog.inv([(V, 1, 1)])
    prog.inv([(V, 0, 1)] * 256 + [(V, 0, N - 256)])                # 256 x - 256 x
    prog.inv([(V, 1, N - 1), (ONE, 0, 3)])
    prog.inv([(V, 1, 1 << 251)] * 200 + [(ONE, 0, 1)] * 57)
    prog.mul([(R, 0, 1), (R, 2, 1)], [(O, 4, 1), (R, 4, 1)])
    prog.end_phase1()
    return wc.Case("inv_long", prog, [([N - 1, 5], (), ()), ([1 << 251, 3], (), ()), ([0, 0], (), ())])


DEPTH = 8


def deep_case():
    """an INV gate that reads a_O of a lower level, then a chain of DEPTH INV gates each reading the previous a_O (one gate a level:
    nothing to batch), the a_O in {0, 1} shifted so that some links are zero"""
    prog = Program(DEPTH + 2)
    g = prog.mul([(V, 0, 1)], [(V, 1, 1)])
    last = prog.inv([(O, g, 1), (ONE, 0, N - 6)])                  # v_0 v_1 - 6
    for k in range(DEPTH):
        last = prog.inv([(O, last, 1), (V, 2 + k, 1)])
    prog.mul([(R, last, 1)], [(O, last, 1), (ONE, 0, 1)])
    prog.end_phase1()
    rnd = random.Random(88)
    provers = [([2, 3] + [rnd.choice((0, N - 1, 5)) for _ in range(DEPTH)], (), ()) for _ in range(4)]
    provers.append(([7, 9] + [N - 1] * DEPTH, (), ()))
    return wc.Case("inv_deep", prog, provers)


def chi_case():
    """INV gates in phase 2 whose rows carry the challenge: chi v_0 alone (zero for chi = 0), a constant plus a chi part, and one that
    reads phase 1 through chi; a wide phase-2 level so that the batched path meets the challenge too"""
    prog = Program(3, nchi=1)
    prog.mul([(V, 0, 1)], [(V, 1, 1)])
    prog.inv([(V, 2, 1)])
    prog.end_phase1()
    prog.inv([(V, 0, (None, 1))])
    prog.inv([(V, 1, (3, 5)), (O, 0, (None, N - 1))])
    prog.inv([(ONE, 0, (1, 1))])                                   # 1 + chi: zero for chi = N - 1
    for k in range(300):
        prog.inv([(V, k % 3, (k, 1)), (R, 1, (None, k + 1))])
    last = prog.inv([(O, 2, (1, None)), (ONE, 0, (None, 1))])      # a_O + chi, one level up
    prog.mul([(R, last, 1)], [(O, last, 1)])
    rnd = random.Random(99)
    provers = [([rnd.randrange(1, N), rnd.randrange(1, N), rnd.randrange(1, N)], (), (chi,)) for chi in wc.CHIS + (rnd.randrange(N),)]
    provers.append(([0, 5, 0], (), (7,)))
    return wc.Case("inv_chi", prog, provers)


HEAD_MEMBERS = 20


def head_case():
    """an INV gate heading a product chain of HEAD_MEMBERS members, and beside it an INV gate that would qualify as a member (its
    row is one a_O term of its phase) and stays ordinary, with a MUL member linking to ITS a_O"""
    prog = Program(HEAD_MEMBERS + 3)
    last = prog.inv([(V, 0, 1)])
    for k in range(HEAD_MEMBERS):
        last = prog.mul([(O, last, 3)], [(V, 1 + k, 1)]) if k % 2 else prog.mul([(V, 1 + k, 1)], [(O, last, N - 1)])
    g = prog.mul([(V, 1, 1)], [(V, 2, 1)])
    stays = prog.inv([(O, g, 1)])                                  # the first gate on g's a_O, but no MUL: no member
    prog.mul([(O, g, 1)], [(V, 3, 1)])                             # ... so this one is g's member
    prog.mul([(O, stays, 5)], [(V, 4, 1)])                         # a MUL member linking to an INV gate's a_O
    prog.end_phase1()
    rnd = random.Random(20)
    provers = [([x] + [rnd.randrange(1, N) for _ in range(HEAD_MEMBERS + 2)], (), ()) for x in (5, 0, N - 1)]
    return wc.Case("inv_head", prog, provers)


AFFINE_MEMBERS = 18


def affine_case():
    """an affine chain of AFFINE_MEMBERS members linking to an INV gate's a_O"""
    prog = Program(AFFINE_MEMBERS + 2)
    last = prog.inv([(V, 0, 1), (ONE, 0, N - 4)])
    for k in range(AFFINE_MEMBERS):
        last = prog.mul([(O, last, 1 + k), (V, 1 + k, 1)], [(V, 2 + k, 1)])
    prog.end_phase1()
    rnd = random.Random(18)
    provers = [([x] + [rnd.randrange(N) for _ in range(AFFINE_MEMBERS + 1)], (), ()) for x in (9, 4, 0)]
    return wc.Case("inv_affine", prog, provers)


# ---- the is-zero gadget ----------------------------------------------------------------------------------------------------------------
def is_zero_gates(prog, x_row):
    """(x, x^-1) with x x^-1 = b, then (1 - b) x = 0 -> the INV gate (its a_O is b: 1 for a non-zero x)"""
    g = prog.inv(x_row)
    prog.mul([(ONE, 0, 1), (O, g, N - 1)], x_row)
    return g


def is_zero_gadget(cs, x_lc, claim_lc, wrong_inverse=False):
    """the same on a constraint system of the model: allocate_multiplier((x, x^-1)), L = x, the product of (1 - b) and x constrained
    to zero, and b equal to the committed claim"""
    x = cs.eval(x_lc)
    x_inv = inv_or_zero(x)
    if wrong_inverse and x:
        x_inv = (x_inv + 1) % N
    left, _, b = cs.allocate_multiplier((x, x_inv))
    cs.constrain(pm.lc_sub(x_lc, pm.lc_var(left)))
    _, _, out = cs.multiply(pm.lc_sub(pm.lc_const(1), pm.lc_var(b)), x_lc)
    cs.constrain(pm.lc_var(out))
    cs.constrain(pm.lc_sub(pm.lc_var(b), claim_lc))


IS_ZERO_COUNT = 16


def _is_zero_values(rnd, count):
    xs = [rnd.choice((0, 0, 1, N - 1, rnd.randrange(1, N))) for _ in range(count)]
    return xs + [int(x != 0) for x in xs]


def is_zero_case():
    """IS_ZERO_COUNT committed values with zeros among them and as many committed claims `x_j is not zero`; the breaker commits
    to the opposite claim for x_0"""
    count = IS_ZERO_COUNT
    prog = Program(2 * count)
    for j in range(count):
        is_zero_gates(prog, [(V, j, 1)])
    prog.end_phase1()
    rnd = random.Random(160)
    provers = [(_is_zero_values(rnd, count), (), ()) for _ in range(4)]
    provers.append(([0] * count + [0] * count, (), ()))

    def gadget(cs, var, v, inputs, wrong_inverse=False):
        for j in range(count):
            is_zero_gadget(cs, pm.lc_var(var[j]), pm.lc_var(var[count + j]), wrong_inverse)
    return wc.Case("inv_is_zero", prog, provers, gadget, breaker=lambda v, inputs: (list(v[:count]) + [1 - v[count]] + list(v[count + 1:]), inputs))


TWO_PHASE_K, TWO_PHASE_ZEROS = 3, 4


def two_phase_case():
    """phase 1: the is-zero gadget on TWO_PHASE_ZEROS committed values; phase 2: a TWO_PHASE_K-shuffle of the next values
    (witness_cases._shuffle_gates) and one INV gate whose row carries the challenge, v_0 - z"""
    k, cnt = TWO_PHASE_K, TWO_PHASE_ZEROS
    base = 2 * cnt
    prog = Program(base + 2 * k, nchi=1)
    for j in range(cnt):
        is_zero_gates(prog, [(V, j, 1)])
    prog.end_phase1()
    wc._shuffle_gates(prog, k, base)
    prog.inv([(V, 0, 1), (ONE, 0, (None, N - 1))])
    rnd = random.Random(230)
    provers = [(_is_zero_values(rnd, cnt) + wc._shuffle_values(rnd, k), (), (chi,)) for chi in wc.CHIS + (rnd.randrange(N), rnd.randrange(N))]

    def gadget(cs, var, v, inputs):
        for j in range(cnt):
            is_zero_gadget(cs, pm.lc_var(var[j]), pm.lc_var(var[cnt + j]))
        pm.shuffle_gadget(cs, var[base:base + k], var[base + k:])

        def cb(cs):
            z = cs.challenge_scalar(LABEL)
            x_lc = pm.lc_add(pm.lc_var(var[0]), pm.lc_const(-z))
            x = cs.eval(x_lc)
            left, _, _ = cs.allocate_multiplier((x, inv_or_zero(x)))
            cs.constrain(pm.lc_sub(x_lc, pm.lc_var(left)))
        cs.specify_randomized_constraints(cb)
    return wc.Case("inv_two_phase", prog, provers, gadget,
                   breaker=lambda v, inputs: (list(v[:cnt]) + [1 - v[cnt]] + list(v[cnt + 1:]), inputs))


def gadget_cases():
    return [c for c in cases() if c.gadget is not None]


CHAINED = ("inv_head", "inv_affine", "inv_two_phase")          # the cases with a chain: run with the scan form enabled too
_cases = None


def cases():
    """every case, built once"""
    global _cases
    if _cases is None:
        _cases = ([level_case(size) for size in LEVEL_SIZES] +
                  [edge_values_case(), long_row_case(), deep_case(), chi_case(), head_case(), affine_case(), is_zero_case(), two_phase_case()])
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)
