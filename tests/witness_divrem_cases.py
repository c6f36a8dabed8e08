"""Gate programs with BPGPU_GATE_DIVREM gates (include/bpgpu.h: x, y the canonical integers of the two rows; a_L = x // y, a_R = x % y,
or 0 and x for y = 0; a_O = a_L a_R) on the Program of tests/witness_inv_cases.py: the op, its evaluation on Python integers
(divmod), operands on every word boundary of a shifting or a schoolbook division, rows that are the heaviest lazy sums, and the
div-rem gadget with its range check run on the model prover.  The reference of every test: computed once per case and left
unchanged.  self_check() asserts that each case contains what it claims.  No GPU."""
import random

import lazy_sum_cases as lz
import witness_affine_cases as af
import witness_chain_cases as cc
import witness_cases as wc
import witness_inv_cases as ic

pm = wc.pm
N = wc.N
L, R, O, V, ONE = wc.L, wc.R, wc.O, wc.V, wc.ONE
DIVREM = 6                                            # BPGPU_GATE_DIVREM; 3 and 5 are no ops
LABEL = wc.SHUFFLE_LABEL
LANE_MAX = wc.LANE_MAX


def divrem(x, y):
    """the op on canonical integers: the identity x = q y + r holds for y = 0 too"""
    return divmod(x, y) if y else (0, x)


class Program(ic.Program):
    def divrem(self, left, right):
        return self._add(DIVREM, 0, left, right)

    def evaluate(self, v, inputs=(), chi=(), phase=0, planes=None):
        """the witness on integers, ops 4 and 6 included -> (a_L, a_R, a_O); phase 2 continues the planes given"""
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
            elif op == ic.INV:
                aL[i] = ev(left)
                aR[i] = ic.inv_or_zero(aL[i])
            elif op == DIVREM:
                aL[i], aR[i] = divrem(ev(left), ev(right))
            else:
                aL[i], aR[i] = ev(left), ev(right)
            aO[i] = aL[i] * aR[i] % N
        return aL, aR, aO

    def operands(self, v, chi=()):
        """[(gate, x, y)] of the DIVREM gates on a prover: what their rows evaluate to, from the planes below each gate"""
        aL, aR, aO = self.evaluate(v, (), chi)
        plane = (aL, aR, aO, v)

        def ev(row):
            tot = 0
            for kind, idx, coeff in row:
                c = sum((part or 0) * (chi[j - 1] if j else 1) for j, part in enumerate(self.parts(coeff)))
                tot += c * (1 if kind == ONE else plane[kind][idx])
            return tot % N
        return [(i, ev(g[2]), ev(g[3])) for i, g in enumerate(self.gates) if g[0] == DIVREM]


def _pairs_program(count):
    """gate k = divrem(v_{2k}, v_{2k+1}), one level"""
    prog = Program(2 * count)
    for k in range(count):
        prog.divrem([(V, 2 * k, 1)], [(V, 2 * k + 1, 1)])
    prog.end_phase1()
    return prog


# ---- operands at the edges -----------------------------------------------------------------------------------------------------------
EDGES = (0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 251, (N + 1) // 2, N - 1)


def edges_case():
    """all ordered pairs of EDGES as committed values, one level"""
    prog = Program(len(EDGES))
    for i in range(len(EDGES)):
        for j in range(len(EDGES)):
            prog.divrem([(V, i, 1)], [(V, j, 1)])
    prog.end_phase1()
    return wc.Case("dr_edges", prog, [(list(EDGES), (), ())])


BITLENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 251, 252)


def bitlen_values(ones):
    """a value of every bit length of BITLENS: 2^b - 1 (ones) or 2^(b - 1); 2^252 - 1 is above n, so 252 bits of ones are n - 1"""
    return [((1 << b) - 1 if b < 252 else N - 1) if ones else 1 << (b - 1) for b in BITLENS]


def bitlen_case():
    """every ordered pair of bit lengths, once on all-ones values and once on powers of two (the two provers)"""
    prog = Program(len(BITLENS))
    for i in range(len(BITLENS)):
        for j in range(len(BITLENS)):
            prog.divrem([(V, i, 1)], [(V, j, 1)])
    prog.end_phase1()
    return wc.Case("dr_bitlen", prog, [(bitlen_values(True), (), ()), (bitlen_values(False), (), ())])


DIGIT_TOPS = (0x80000000, 0xFFFFFFFF, 0x00000001)
ONES32 = 0xFFFFFFFF


def digit_pairs():
    """(x, y) that drive a schoolbook division into its correction step: the divisor's top word from DIGIT_TOPS with the next word 0
    or all-ones, 2 to 4 words long; the dividend's leading words those of the divisor, zero middle words below them, then a low
    word; equal operands, and x = y +- 1"""
    rnd = random.Random(606)
    pairs = []
    for top in DIGIT_TOPS:
        for nxt in (0, ONES32):
            for words in (2, 3, 4):
                low = [rnd.getrandbits(32) for _ in range(words - 2)]
                y = sum(w << (32 * k) for k, w in enumerate(low + [nxt, top]))
                lead = top << 32 | nxt
                for xwords in range(words, 8):
                    for tail in (0, ONES32):
                        x = lead << (32 * (xwords - 2)) | tail
                        if x < N:
                            pairs.append((x, y))
                            if not tail:
                                pairs.append((x - 1, y))
                pairs += [(y, y), (y + 1, y), (y - 1, y)]
    return pairs


def digits_case():
    pairs = digit_pairs()
    return wc.Case("dr_digits", _pairs_program(len(pairs)), [([t for pair in pairs for t in pair], (), ())])


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 16, 17, 65)
QUOTIENT_DEPTH = 4


def rows_case():
    """rows of every length of ROW_LENGTHS on either side (65 terms: a wave sums the row and lane 0 divides), over the committed
    values, the constant and a_L / a_R / a_O of the gates below, DIVREM gates among them; a quotient of a quotient QUOTIENT_DEPTH
    levels deep; and a DIVREM gate whose rows have the product-link shape (one a_O term of its phase, the other row free of the
    phase's multipliers) that must stay an ordinary gate"""
    rnd = random.Random(65)
    prog = Program(6)
    prog.mul([(V, 0, 1)], [(V, 1, 1)])                              # gate 0
    prog.divrem([(V, 2, 1)], [(V, 3, 1)])                           # gate 1
    prog.divrem([(O, 0, 1), (V, 4, 1)], [(R, 1, 1), (ONE, 0, 1)])   # gate 2
    prog.link_shaped = prog.divrem([(O, 0, 1)], [(V, 4, 1)])        # a_O of gate 0, which has no member: as a MUL this were one

    def row(i, length):
        out = []
        for _ in range(length):
            kind = rnd.choice((V, V, ONE, L, R, O))
            idx = 0 if kind == ONE else (rnd.randrange(prog.m) if kind == V else rnd.randrange(i))
            out.append((kind, idx, rnd.choice((1, 1, 2, (1 << 32) + 1, N - 1, rnd.randrange(N)))))
        return out
    for ll in ROW_LENGTHS:
        for rl in ROW_LENGTHS:
            i = prog.n
            prog.divrem(row(i, ll), row(i, rl))
    last = prog.divrem([(V, 5, 1)], [(V, 3, 1)])                    # the quotient of a quotient ...
    for _ in range(QUOTIENT_DEPTH - 1):
        last = prog.divrem([(L, last, 1)], [(V, 4, 1)])
    prog.end_phase1()
    provers = []
    for _ in range(3):
        v = [rnd.getrandbits(rnd.choice((16, 64, 130, 250))) for _ in range(4)] + [rnd.getrandbits(20) + 2, rnd.randrange(N // 2, N)]
        provers.append((v, (), ()))
    return wc.Case("dr_rows", prog, provers)


LAZY_LENGTHS = (1, 16, 17, 33, 64, 65)


def lazy_case():
    """operand rows whose every product is lazily n - 1 (coefficient x value = lz.C: tests/lazy_sum_cases.py), straight and through
    chi, on either side; one such sum that is exactly zero as the divisor and one that is exactly n - 1.  The quotient is right only
    if the row was brought to its canonical integer"""
    rnd = random.Random(2027)
    vals = [rnd.randrange(1, N) for _ in range(4)] + [rnd.getrandbits(100) + 1]
    chi = (rnd.randrange(1, N),)
    prog = Program(len(vals), nchi=1)
    prog.end_phase1()
    for length in LAZY_LENGTHS:
        worst = [(V, 3, lz.C * lz.inv(vals[3]) % N)] * length
        mixed = [(V, k % 4, lz.C * lz.inv(vals[k % 4]) % N) for k in range(length)]
        through_chi = [(V, 2, (None, lz.C * lz.inv(vals[2] * chi[0]) % N))] * length
        prog.divrem(worst, [(V, 4, 1)])
        prog.divrem([(ONE, 0, N - 1)], worst)
        prog.divrem(mixed, through_chi)
        prog.divrem(through_chi, mixed + [(V, 4, 1)])
        prog.divrem(worst, worst + [(ONE, 0, -length * lz.C % N)])                  # the divisor: the heaviest sum that is zero
        prog.divrem(worst + [(ONE, 0, (N - 1 - length * lz.C) % N)], [(V, 4, 1)])    # the dividend: exactly n - 1
    return wc.Case("dr_lazy", prog, [(vals, (), chi)])


LEVEL = 257
LEVEL_ZEROS = (0, 256)          # thread 0's first and second gate; the second is also the level's last


def level_case():
    """one level of LEVEL gates, gate i = divrem(v_0 + i 2^40, d_i): a ragged second round of the 256 threads, with a zero divisor
    (a constant term with the coefficient 0) at LEVEL_ZEROS"""
    rnd = random.Random(257)
    prog = Program(2)
    for i in range(LEVEL):
        d = 0 if i in LEVEL_ZEROS else rnd.getrandbits(rnd.choice((8, 33, 64, 100)))
        prog.divrem([(V, 0, 1), (ONE, 0, i << 40)], [(ONE, 0, d), (V, 1, 1)])
    prog.end_phase1()
    return wc.Case("dr_level257", prog, [([rnd.getrandbits(200), 0], (), ()), ([N - 1 - (256 << 40), 0], (), ()), ([5, 1], (), ())])


TWO_PHASE_K = 3


def two_phase_case():
    """nchi = 1.  Phase 1: TWO_PHASE_K products v_0 v_{2+k}.  Phase 2, for each k: g = divrem(chi v_0 + a_O[k], v_1) with
    h = multiply(a_L[g], v_1) for the circuit's q y, and g' = divrem(chi v_0 + a_O[k], chi)"""
    k = TWO_PHASE_K
    prog = Program(2 + k, nchi=1)
    for j in range(k):
        prog.mul([(V, 0, 1)], [(V, 2 + j, 1)])
    prog.end_phase1()
    for j in range(k):
        x = [(V, 0, (None, 1)), (O, j, 1)]
        g = prog.divrem(x, [(V, 1, 1)])
        prog.mul([(L, g, 1)], [(V, 1, 1)])
        prog.divrem(x, [(ONE, 0, (None, 1))])
    rnd = random.Random(232)
    provers = []
    for chi in wc.CHIS + (rnd.randrange(N),):
        provers.append(([rnd.getrandbits(60), rnd.getrandbits(90) + 1] + [rnd.getrandbits(64) for _ in range(k)], (), (chi,)))
    return wc.Case("dr_two_phase", prog, provers)


def two_phase_circuit():
    """the constraints of dr_two_phase as rows of (variable, coefficient) terms, a coefficient (c0, c1) standing for c0 + chi c1:
    every multiplier bound to its rows, x = q v_1 + r through the product gate, and x = q chi + r -> (q, nchi, row_ptr, kind, idx,
    coeff) of bpgpu_circuit_create_param, and the rows themselves"""
    k = TWO_PHASE_K
    rows = []
    for j in range(k):
        rows.append([(("L", j), 1), (("V", 0), N - 1)])
        rows.append([(("R", j), 1), (("V", 2 + j), N - 1)])
    for j in range(k):
        g, h, g2 = k + 3 * j, k + 3 * j + 1, k + 3 * j + 2
        x = [(("V", 0), (None, 1)), (("O", j), 1)]
        rows.append([(("L", h), 1), (("L", g), N - 1)])
        rows.append([(("R", h), 1), (("V", 1), N - 1)])
        rows.append(x + [(("O", h), N - 1), (("R", g), N - 1)])                  # x - q v_1 - r
        rows.append(x + [(("L", g2), (None, N - 1)), (("R", g2), N - 1)])        # x - chi q' - r'
    rp, kd, ix, cf, _ = wc.md.circuit_rows(rows, nchi=1)
    return (len(rows), 1, rp, kd, ix, cf), rows


def rows_hold(rows, planes, v, chi):
    """the first row of a (variable, coefficient) circuit that does not vanish on a witness, or -1"""
    value = {"L": planes[0], "R": planes[1], "O": planes[2], "V": v}
    for r, row in enumerate(rows):
        tot = 0
        for var, c in row:
            c = sum((part or 0) * (chi[j - 1] if j else 1) for j, part in enumerate(c)) if isinstance(c, tuple) else c
            tot += c * (1 if var[0] == "1" else value[var[0]][var[1]])
        if tot % N:
            return r
    return -1


HEAD_MEMBERS, AFFINE_MEMBERS = 20, 18


def head_case():
    """a DIVREM gate heading a product chain of HEAD_MEMBERS MUL members that link to its a_O, and another heading an affine chain
    of AFFINE_MEMBERS"""
    prog = Program(HEAD_MEMBERS + AFFINE_MEMBERS + 4)
    last = prog.divrem([(V, 0, 1)], [(V, 1, 1)])
    for k in range(HEAD_MEMBERS):
        last = prog.mul([(O, last, 3)], [(V, 2 + k, 1)]) if k % 2 else prog.mul([(V, 2 + k, 1)], [(O, last, N - 1)])
    base = 2 + HEAD_MEMBERS
    prog.affine_head = last = prog.divrem([(V, 1, 1), (ONE, 0, 77)], [(V, 0, 1)])
    for k in range(AFFINE_MEMBERS):
        last = prog.mul([(O, last, 1 + k), (V, base + k, 1)], [(V, base + 1 + k, 1)])
    prog.end_phase1()
    rnd = random.Random(2018)
    provers = []
    for x, y in ((1 << 70 | 12345, 1000003), (5, 0), (N - 1, 2)):
        provers.append(([x, y] + [rnd.randrange(1, N) for _ in range(HEAD_MEMBERS + AFFINE_MEMBERS + 2)], (), ()))
    return wc.Case("dr_head", prog, provers)


# ---- the div-rem gadget ----------------------------------------------------------------------------------------------------------------
GADGET_BITS = 16


def divrem_gadget(cs, a, b, va, vb):
    """q = a // b and r = a % b allocated as ONE multiplier (allocate twice: prover.rs:127-146), q b through a product,
    a = q b + r, and the range check r < b as r in [0, 2^16) and b - 1 - r in [0, 2^16)"""
    q, r = divrem(va % N, vb % N)
    lq = cs.allocate(q)
    rr = cs.allocate(r)
    _, _, qb = cs.multiply(pm.lc_var(lq), pm.lc_var(b))
    cs.constrain(pm.lc_sub(pm.lc_add(pm.lc_var(qb), pm.lc_var(rr)), pm.lc_var(a)))
    pm.range_proof_gadget(cs, pm.lc_var(rr), r, GADGET_BITS)
    gap = pm.lc_sub(pm.lc_sub(pm.lc_var(b), pm.lc_const(1)), pm.lc_var(rr))
    pm.range_proof_gadget(cs, gap, (vb - 1 - r) % N, GADGET_BITS)


GADGET_PROVERS = ((40000, 1), (123, 4567), (51 * 1285, 1285), (65534, 65535), (777, 0))       # b = 1, b > a, b | a, b = 2^16 - 1, b = 0


def gadget_case():
    """committed a, b in 16 bits: gate 0 = divrem(a, b), gate 1 = multiply(a_L[0], b), 16 BIT gates on a_R[0] and 16 on
    b - 1 - a_R[0]; the prover with b = 0 is rejected by the range check"""
    prog = Program(2)
    g = prog.divrem([(V, 0, 1)], [(V, 1, 1)])
    prog.mul([(L, g, 1)], [(V, 1, 1)])
    for i in range(GADGET_BITS):
        prog.bit([(R, g, 1)], i)
    for i in range(GADGET_BITS):
        prog.bit([(V, 1, 1), (ONE, 0, N - 1), (R, g, N - 1)], i)
    prog.end_phase1()

    def gadget(cs, var, v, inputs):
        divrem_gadget(cs, var[0], var[1], v[0], v[1])
    return wc.Case("dr_gadget", prog, [(list(p), (), ()) for p in GADGET_PROVERS], gadget)


def gadget_verdict(case, p):
    """(ok, first_bad_row, first_bad_gate) of prover p of a gadget case, from the model prover's constraints"""
    pv = case.model(p)
    row = next((r for r, lc in enumerate(pv.constraints) if pv.eval(lc)), -1)
    gate = next((i for i in range(len(pv.a_L)) if pv.a_L[i] * pv.a_R[i] % N != pv.a_O[i]), -1)
    return int(row < 0 and gate < 0), row, gate


CHAINED = ("dr_head",)                                # the cases with a chain: run with the scan form enabled too
_cases = None


def cases():
    """every case, built once"""
    global _cases
    if _cases is None:
        _cases = [edges_case(), bitlen_case(), digits_case(), rows_case(), lazy_case(), level_case(), two_phase_case(), head_case(),
                  gadget_case()]
        assert max(c.prog.n for c in _cases) <= 600
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


def gate_operands(case, p):
    """per DIVREM gate of the case: (gate, x, y) on prover p"""
    v, _, chi = case.prover(p)
    return case.prog.operands(v, chi)


def self_check():
    """each case contains what it claims"""
    for c in cases():
        assert any(g[0] == DIVREM for g in c.prog.gates), c.name
        for p in range(len(c.provers)):
            aL, aR, aO = c.want(p)
            for i, x, y in gate_operands(c, p):
                assert x == aL[i] * y + aR[i] and (y == 0 or aR[i] < y) and (y != 0 or aL[i] == 0), (c.name, p, i)
    # dr_edges: all ordered pairs, one level
    e = case("dr_edges")
    assert {(x, y) for _, x, y in gate_operands(e, 0)} == {(x, y) for x in EDGES for y in EDGES} and e.prog.levels()[:3] == (1, 0, 144)
    assert len(EDGES) == 12 and all(x < N for x in EDGES)
    # dr_bitlen: every ordered pair of bit lengths, on both kinds of value
    b = case("dr_bitlen")
    for p, ones in ((0, True), (1, False)):
        ops = gate_operands(b, p)
        assert {(x.bit_length(), y.bit_length()) for _, x, y in ops} == {(s, t) for s in BITLENS for t in BITLENS}
        assert all(((x & (x + 1)) == 0 or x == N - 1) if ones else (x & (x - 1)) == 0 for _, x, _ in ops)
    # dr_digits: the top words, the next words, equal operands and x = y +- 1
    pairs = digit_pairs()
    assert [(x, y) for _, x, y in gate_operands(case("dr_digits"), 0)] == pairs and all(x < N and 0 < y < N for x, y in pairs)
    tops = {(y >> (32 * ((y.bit_length() - 1) // 32)), (y >> (32 * ((y.bit_length() - 1) // 32 - 1))) & ONES32) for _, y in pairs}
    assert tops == {(t, nxt) for t in DIGIT_TOPS for nxt in (0, ONES32)}
    assert any(x == y for x, y in pairs) and any(x == y + 1 for x, y in pairs) and any(x == y - 1 for x, y in pairs)
    assert any(x.bit_length() > 192 and (x >> 64) & ((1 << 64) - 1) == 0 for x, _ in pairs)            # zero middle words
    # dr_rows: the row lengths on either side, reads of all three planes of DIVREM gates, the depth, and the link shape
    r = case("dr_rows")
    prog = r.prog
    lens = {(prog.row_len(g[2]), prog.row_len(g[3])) for g in prog.gates if g[0] == DIVREM}
    assert lens >= {(s, t) for s in ROW_LENGTHS for t in ROW_LENGTHS} and prog.levels()[3] == 2 * len(ROW_LENGTHS)
    read = {kind for g in prog.gates for kind, idx, _ in g[2] + g[3] if kind <= O and prog.gates[idx][0] == DIVREM}
    assert read == {L, R, O}
    depth = [0] * prog.n
    for i, g in enumerate(prog.gates):
        if g[0] == DIVREM:
            depth[i] = 1 + max([depth[idx] for kind, idx, _ in g[2] if kind == L] + [0])
    assert max(depth) >= QUOTIENT_DEPTH
    assert any(y == 0 for p in range(len(r.provers)) for _, _, y in gate_operands(r, p))                # the empty right rows
    pred = cc.analyse(prog)[0]
    as_mul = Program(prog.m)
    as_mul.gates = [(wc.MUL if g[0] == DIVREM else g[0],) + g[1:] for g in prog.gates]
    as_mul.n1 = prog.n1
    assert pred[prog.link_shaped] is None and cc.analyse(as_mul)[0][prog.link_shaped] == 0
    # dr_lazy: every product of a `worst` row is n - 1 lazily; a zero divisor and a dividend n - 1 come out of such sums
    z = case("dr_lazy")
    vals = z.provers[0][0]
    assert z.prog.gates[0][2][0][2] * vals[3] % N == lz.C
    ops = gate_operands(z, 0)
    assert sum(1 for _, _, y in ops if y == 0) == len(LAZY_LENGTHS) and sum(1 for _, x, _ in ops if x == N - 1) >= len(LAZY_LENGTHS)
    assert any(z.prog.row_len(g[2]) > LANE_MAX for g in z.prog.gates) and any(z.prog.row_len(g[3]) > LANE_MAX for g in z.prog.gates)
    # dr_level257: one level, the zero divisors where thread 0 meets them and at the end
    lv = case("dr_level257")
    assert lv.prog.levels()[:3] == (1, 0, LEVEL) and LEVEL_ZEROS == (0, 256) and LEVEL - 1 in LEVEL_ZEROS
    assert [i for i, _, y in gate_operands(lv, 0) if y == 0] == list(LEVEL_ZEROS)
    # dr_two_phase: the challenges, the operands, and the circuit holds for every prover
    t = case("dr_two_phase")
    assert [pr[2][0] for pr in t.provers[:3]] == [0, 1, N - 1] and len(t.provers) == 4 and t.prog.nchi == 1
    _, rows = two_phase_circuit()
    for p, (v, _, chi) in enumerate(t.provers):
        assert rows_hold(rows, t.want(p), v, chi) == -1, p
        ops = gate_operands(t, p)
        assert all(i >= t.prog.phase1 for i, _, _ in ops)
        assert {y for _, _, y in ops} == {v[1], chi[0]} and all(x == (chi[0] * v[0] + t.want(p)[2][j]) % N for j in range(TWO_PHASE_K) for _, x, _ in ops[2 * j:2 * j + 2])
    # dr_head: the chains
    h = case("dr_head").prog
    pred, _, figs = cc.analyse(h)
    assert h.gates[0][0] == DIVREM and pred[0] is None and pred[1] == 0 and figs["longest"][0] == HEAD_MEMBERS
    a = af.figures(h)
    assert h.gates[h.affine_head][0] == DIVREM and a["affine1"] == AFFINE_MEMBERS and a["chains1"] == 2
    # dr_gadget: the program is the model prover's witness, and the verdicts
    g = case("dr_gadget")
    verdicts = []
    for p, (a_, b_) in enumerate(GADGET_PROVERS):
        pv = g.model(p)
        assert (pv.a_L, pv.a_R, pv.a_O) == tuple(g.want(p)) and len(pv.a_L) == g.prog.n == 2 + 2 * GADGET_BITS
        verdicts.append(gadget_verdict(g, p))
        assert verdicts[-1][2] == -1
    assert [ok for ok, _, _ in verdicts] == [1, 1, 1, 1, 0]
    b1, bgt, bdiv, bmax, bzero = GADGET_PROVERS
    assert b1[1] == 1 and bgt[1] > bgt[0] and bdiv[0] % bdiv[1] == 0 and bmax[1] == (1 << 16) - 1 and bzero[1] == 0
    # the rejected prover fails in the range check of b - 1 - r: its last row, the recomposition
    assert verdicts[4][1] == len(g.model(4).constraints) - 1
