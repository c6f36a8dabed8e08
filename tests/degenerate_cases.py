"""Proofs whose points coincide, and a CPU shadow of the order in which the verification kernels add them.  Test infrastructure,
no GPU: tests/test_degenerate_cases.py checks it, tests/test_gpu_degenerate_points.py drives the kernels with it.

The point arithmetic of csrc/ec29.cuh keeps the exact cases of the group law -- P + P, P + (-P), an accumulator that has become
the identity, a doubling of the identity -- in cold out-of-line functions which honest operands practically never reach.  A
prover chooses the proof points, so here they are chosen to coincide:

  twin      A_O1 := A_I1, T_3 := T_1, R_j := L_j
  opposite  A_O1 := -A_I1, T_3 := -T_1, R_j := -L_j
  line      every proof point that is not the identity, and V_0, := m_i * P with one random point P per proof, m_i in +-{1..mmax}
  line_B    the same with P = the Pedersen base B
  gens      A_I1 := B, A_O1 := B_blinding, S1 := G_0, T_1 := H_0, V_0 := G_1, L_0 := G_0, R_0 := -H_0

(identity points never go into the slots the transcript validates: the reference rejects those before any MSM).  The scalars of
such a proof are whatever the transcript replay over the crafted points gives: the oracle's VerifySession is the reference.

The shadow gives every proof point a (class, multiplier): points of one class are known multiples of one point, points of
different classes are unrelated.  A partial sum is then a map class -> integer mod n, and walking the kernels' addition order
with these maps tells when an addition meets one of the exact cases:

  dbl     acc == addend                     (the P = Q branch of the *_full functions)
  cancel  acc == -addend                    (the sum is the identity)
  ident   the addend meets an identity accumulator
  dbl0    a doubling of an identity accumulator

Three orders (csrc/k_ec.hip, host routing in csrc/bpgpu_api.hip verify_straus_args):
  (a) straus_body<NP>: lane l of a proof holds the points l + j * (nvar / NP), j < NP; windows descending, 4 doublings between
      them, the lane's points ascending within a window.  Every lane starts at the identity, so `ident` and `dbl0` count only
      once the lane has held a point: an identity its own additions produced.
  (b) k_verify_windows: lane w adds d_{v,w} * P_v over the proof's points in ascending order; no doublings, so `dbl0` cannot
      occur in this order.  `ident` as in (a).
  (c) the two Horner stages over the 64 window sums S_w of (b): groups of 8 (acc = S_{8g+7}; 4 doublings, + S_{8g+i} for
      i = 6..0), then the 8 group sums (32 doublings between them).  Both operands come from memory, so `ident` and `dbl0`
      count from the first operation on.  All of this batch's cases fall into the first stage: the second stage meets one only
      if a whole group of 8 window sums vanishes or 2^32 T_g = +-T_{g-1}, which transcript-derived scalars do not give at any
      rate a seed search can find (about 2^-38 per `line` proof with every point +-P).  Only a caller who chooses the scalars
      reaches them: the plain MSM entry points, whose tests feed such inputs (test_gpu_parity.py).
The lane, quad (ec29_quad.cuh) and row (ec29_row.cuh) forms of (c) run the same sequence of group operations -- q4_dbl / q4_add
and rdbl / radd stand where jac_dbl / jac_add stand, in the same loops -- so one shadow serves the three.
"""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

import bp_helpers as bh
import oracle_lib as o

N, P_MOD = o.N, o.P
IDENT = bytes(64)
KINDS = ("twin", "opposite", "line", "line_B", "gens")
EVENTS = ("dbl", "cancel", "ident", "dbl0")
LABEL = b"RangeProofTest"
FIRST11 = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6")


# ------------------------------------------------------------------ points as bytes
def pt_neg(pt):
    if pt == IDENT:
        return pt
    return pt[:32] + ((P_MOD - int.from_bytes(pt[32:], "little")) % P_MOD).to_bytes(32, "little")


def small_multiples(pt, mmax=8):
    """{m: m * pt for m in +-1..mmax} by repeated addition"""
    out, acc = {}, IDENT
    for m in range(1, mmax + 1):
        acc = o.point_add(acc, pt)
        out[m], out[-m] = acc, pt_neg(acc)
    return out


# ------------------------------------------------------------------ the flat proof as named 64-byte slots
class Slots:
    """the points of a flat proof (bp_helpers.parse_flat_proof) and its commitments, by name; names() is the operand order of
    bp_helpers.verify_inputs"""

    def __init__(self, proof, com):
        self.proof, self.com = bytearray(proof), bytearray(com)
        self.k, self.m = int.from_bytes(proof[:4], "little"), len(com) // 64
        self.off = {name: 8 + 64 * i for i, name in enumerate(FIRST11)}
        l_off = 8 + 11 * 64 + 96
        for j in range(self.k):
            self.off["L%d" % j] = l_off + 64 * j
            self.off["R%d" % j] = l_off + 64 * (self.k + j)

    def names(self):
        return (list(FIRST11[:6]) + ["V%d" % i for i in range(self.m)] + list(FIRST11[6:])
                + ["L%d" % j for j in range(self.k)] + ["R%d" % j for j in range(self.k)])

    def get(self, name):
        if name[0] == "V":
            i = int(name[1:])
            return bytes(self.com[64 * i:64 * i + 64])
        return bytes(self.proof[self.off[name]:self.off[name] + 64])

    def set(self, name, pt):
        assert len(pt) == 64 and pt != IDENT
        if name[0] == "V":
            i = int(name[1:])
            self.com[64 * i:64 * i + 64] = pt
        else:
            self.proof[self.off[name]:self.off[name] + 64] = pt

    def done(self):
        return bytes(self.proof), bytes(self.com)


def craft(kind, proof, com, seed, mmax=8):
    """-> (proof, commitments, classes): the crafted bytes and, in operand order, each point's (class, multiplier) -- None for an
    identity point.  kind None: the proof as it is."""
    s = Slots(proof, com)
    names = s.names()
    cls = {nm: (nm, 1) for nm in names}
    rnd = random.Random(seed)
    if kind in ("twin", "opposite"):
        sign = 1 if kind == "twin" else -1
        for dst, src in [("A_O1", "A_I1"), ("T_3", "T_1")] + [("R%d" % j, "L%d" % j) for j in range(s.k)]:
            s.set(dst, s.get(src) if sign == 1 else pt_neg(s.get(src)))
            cls[dst] = (src, sign)
    elif kind in ("line", "line_B"):
        base = o.generator() if kind == "line_B" else o.point_mul(o.s2b(rnd.randrange(1, N)), o.generator())
        mult = small_multiples(base, mmax)
        for nm in names:
            if nm == "V0" or (nm[0] != "V" and s.get(nm) != IDENT):
                m = rnd.choice((-1, 1)) * rnd.randrange(1, mmax + 1)
                s.set(nm, mult[m])
                cls[nm] = ("line", m)
    elif kind == "gens":
        G, Hh, B = o.gens("G", 2), o.gens("H", 1), o.generator()     # B == B_blinding (the reference's PedersenGens)
        for nm, pt, c in (("A_I1", B, ("B", 1)), ("A_O1", B, ("B", 1)), ("S1", G[:64], ("G0", 1)), ("T_1", Hh, ("H0", 1)),
                          ("V0", G[64:], ("G1", 1)), ("L0", G[:64], ("G0", 1)), ("R0", pt_neg(Hh), ("H0", -1))):
            s.set(nm, pt)
            cls[nm] = c
    else:
        assert kind is None
    return s.done() + ([None if s.get(nm) == IDENT else cls[nm] for nm in names],)


def tamper_scalar(proof, i):
    bad = bytearray(proof)
    bad[8 + 11 * 64 + (i % 3) * 32] ^= 1 + (i % 7)      # a bit of t_x / t_x_blinding / e_blinding (bp_helpers.make_range_batch)
    return bytes(bad)


class Rec:
    """one proof of a batch with the oracle's verdict on it"""

    def __init__(self, kind, proof, com, classes, n_bits, cap, oracle_kind=o.K_RANGE, label=LABEL):
        self.kind, self.proof, self.com, self.classes = kind, proof, com, classes
        s = o.VerifySession(oracle_kind, n_bits, label, [], com, proof, cap)
        self.k, self.points, self.scalars = bh.verify_inputs(proof, com)
        self.n1, self.m, self.nterms = s.n1, s.m, s.nterms
        self.rc, self.ok = s.rc, 1 if s.rc == 0 else 0
        self.challenges, self.mega, self.full = s.challenges(), s.mega_check(), s.msm_terms()[0]
        self.csr, self.n = s.csr(), s.n1 + s.n2
        s.close()
        self.nvar = 11 + self.m + 2 * self.k

    def var_scalars(self):
        """the scalars of the proof points in operand order, out of the oracle's MSM scalars (the generators' sit between T_6 and L_0)"""
        sc = o.unscalars(self.full)
        head = 11 + self.m
        return sc[:head] + sc[len(sc) - 2 * self.k:]


def make_rec(kind, seed, n_bits=8, mmax=8, tamper=False):
    """the proof of make_range_batch's value for `seed`, crafted as `kind` (craft seed = prove seed)"""
    cap = 1 << max(0, (n_bits - 1).bit_length())
    v = (0x9E3779B97F4A7C15 * (seed + 1)) % (1 << n_bits)
    rc, proof, com = o.r1cs_prove(o.K_RANGE, n_bits, LABEL, [v], seed, cap)
    assert rc == 0
    if tamper:
        proof = tamper_scalar(proof, seed)
    proof, com, classes = craft(kind, proof, com, seed, mmax)
    return Rec("tampered" if tamper else (kind or "honest"), proof, com, classes, n_bits, cap)


# ------------------------------------------------------------------ the committed batches
# `line` proofs as (seed, mmax), found with search_line_seeds below: at random the Horner stages (c) meet P + P or P + (-P) in
# about one proof of 300, so the seeds are those whose shadow says they do (mmax 1: every point is +-P, the window sums stay small)
LINE_SEEDS = ((2046, 1), (2087, 1), (2255, 1), (2342, 1), (2085, 1), (2212, 1), (2215, 1), (2218, 1),
              (1128, 8), (1129, 8), (1130, 8), (1139, 8), (1160, 8), (1161, 8), (1165, 8), (1170, 8), (1173, 8), (1186, 8),
              (1189, 8), (1195, 8), (1196, 8), (1199, 8))
LINE_B_SEEDS = tuple((600 + i, 8) for i in range(6))


def batch_plan(n_bits=8):
    """[(kind, seed, mmax, tamper)] of the 70-proof batch, shuffled: honest, scalar-tampered and all five crafted kinds side by side
    (the table and Straus lanes are role-major, so a wave holds ordinary and degenerate lanes at once)"""
    plan = [(None, 100 + i, 8, False) for i in range(70 - 1 - 5 - 5 - 4 - len(LINE_SEEDS) - len(LINE_B_SEEDS))]
    plan += [(None, 200, 8, True)]
    plan += [("twin", 300 + i, 8, False) for i in range(5)] + [("opposite", 400 + i, 8, False) for i in range(5)]
    plan += [("gens", 500 + i, 8, False) for i in range(4)]
    plan += [("line", s, mm, False) for s, mm in LINE_SEEDS] + [("line_B", s, mm, False) for s, mm in LINE_B_SEEDS]
    assert len(plan) == 70
    random.Random(7070).shuffle(plan)
    return plan


def make_batch(n_bits=8):
    return [make_rec(kind, seed, n_bits, mmax, tamper) for kind, seed, mmax, tamper in batch_plan(n_bits)]


# ------------------------------------------------------------------ signed 4-bit recoding (ec29.cuh recode_add_k<4> / recode_digit<4>)
SW, NWIN = 4, 64
_K = sum(8 << (SW * w) for w in range(NWIN))


def digits(s):
    """64 digits in [-8, 7] with sum d_w 16^w = s"""
    t = s + _K
    return [((t >> (SW * w)) & 15) - 8 for w in range(NWIN)]


# ------------------------------------------------------------------ partial sums as maps class -> integer mod n
def _scaled(c, t):
    return {c[0]: c[1] * t % N}


def _add(a, b):
    r = dict(a)
    for c, v in b.items():
        v = (r.get(c, 0) + v) % N
        if v:
            r[c] = v
        else:
            r.pop(c, None)
    return r


def _neg(a):
    return {c: N - v for c, v in a.items()}


def _dbl(a):
    return {c: 2 * v % N for c, v in a.items()}


class Counter(dict):
    def __init__(self):
        super().__init__((e, 0) for e in EVENTS)

    def add(self, acc, q, counts_ident=True):
        """count the case of acc + q (q not the identity) and return the sum"""
        if not acc:
            if counts_ident:
                self["ident"] += 1
        elif acc == q:
            self["dbl"] += 1
        elif acc == _neg(q):
            self["cancel"] += 1
        return _add(acc, q)

    def dbl(self, acc, counts_ident=True):
        if not acc and counts_ident:
            self["dbl0"] += 1
        return _dbl(acc)

    def merge(self, other):
        for e in EVENTS:
            self[e] += other[e]
        return self


def shadow_straus(rec, np_):
    """(a): the full lanes of straus_body<np_> over one proof (the leftover points take lanes of one point each)"""
    cnt, sc, cl = Counter(), rec.var_scalars(), rec.classes
    dg = [digits(s) for s in sc]
    lanes = rec.nvar // np_
    for l in range(lanes):
        pts = [l + j * lanes for j in range(np_) if cl[l + j * lanes] is not None]
        acc, held = {}, False
        for w in range(NWIN - 1, -1, -1):
            if w != NWIN - 1:
                for _ in range(SW):
                    acc = cnt.dbl(acc, held)
            for v in pts:
                if dg[v][w]:
                    acc = cnt.add(acc, _scaled(cl[v], dg[v][w]), held)
                    held = True
    return cnt


def shadow_windows(rec):
    """(b) -> (events, the 64 window sums)"""
    cnt, sc, cl = Counter(), rec.var_scalars(), rec.classes
    dg = [digits(s) for s in sc]
    sums = []
    for w in range(NWIN):
        acc, held = {}, False
        for v in range(rec.nvar):
            if cl[v] is not None and dg[v][w]:
                acc = cnt.add(acc, _scaled(cl[v], dg[v][w]), held)
                held = True
        sums.append(acc)
    return cnt, sums


def _horner(cnt, terms, ndbl):
    acc = terms[-1]
    for q in reversed(terms[:-1]):
        for _ in range(ndbl):
            acc = cnt.dbl(acc)
        acc = cnt.add(acc, q) if q else acc      # (an identity addend is resolved by a select: none of the four cases)
    return acc


def shadow_horner(sums):
    """(c) -> (events, the proof's variable-base sum)"""
    cnt = Counter()
    groups = [_horner(cnt, sums[8 * g:8 * g + 8], SW) for g in range(8)]
    return cnt, _horner(cnt, groups, 8 * SW)


ORDERS = ("straus2", "straus3", "straus4", "windows", "horner")


def shadow_all(rec):
    """{order: events} of one proof; checks the shadow's own bookkeeping: the Horner result is sum s_v * P_v"""
    wc, sums = shadow_windows(rec)
    hc, total = shadow_horner(sums)
    want = {}
    for s, c in zip(rec.var_scalars(), rec.classes):
        if c is not None:
            want = _add(want, _scaled(c, s))
    assert total == want
    out = {"straus%d" % np_: shadow_straus(rec, np_) for np_ in (2, 3, 4)}
    out["windows"], out["horner"] = wc, hc
    return out


def shadow_batch(recs):
    tot = {od: Counter() for od in ORDERS}
    for r in recs:
        for od, c in shadow_all(r).items():
            tot[od].merge(c)
    return tot


def search_line_seeds(kind, seeds, mmax):
    """how LINE_SEEDS / LINE_B_SEEDS were found: -> [(seed, {order: events})] of the seeds whose `kind` proof meets P + P or
    P + (-P) in a Straus lane or in the Horner stages"""
    hits = []
    for seed in seeds:
        ev = shadow_all(make_rec(kind, seed, 8, mmax))
        if any(ev[od]["dbl"] or ev[od]["cancel"] for od in ("straus2", "straus3", "straus4", "horner")):
            hits.append((seed, ev))
    return hits


# ------------------------------------------------------------------ inner-product proofs with coinciding L, R
_IPP_GENS = {}


def ipp_case(n, seed, kind, p_is_l0=False):
    """operands of InnerProductProof::verify for length n.  The verifier takes P as an input, so any L_j, R_j, a, b make an accepted
    proof once P := the expect_P of these operands: L_j, R_j are random points (kind None) crafted as twin, opposite or line, the
    challenges come from the model's transcript replay over them.  p_is_l0: P := L_0 instead.
    -> the operands, `bit` (the oracle's verdict on P) and `bit_shifted` (its verdict on P + B)"""
    import ipp_verify_cases as cases
    k = n.bit_length() - 1
    if n not in _IPP_GENS:
        _IPP_GENS[n] = cases.gens(n)
    G, H = _IPP_GENS[n]
    a, b, w = (o.random_scalars(seed * 8 + t, 1) for t in range(3))
    Gf, Hf = (o.random_scalars(seed * 8 + 3 + t, n) for t in range(2))
    Q = o.point_mul(w, o.generator())
    rnd = random.Random(seed)

    def some_point():
        return o.point_mul(o.s2b(rnd.randrange(1, N)), o.generator())
    L = [some_point() for _ in range(k)]
    if kind == "twin":
        R = list(L)
    elif kind == "opposite":
        R = [pt_neg(p) for p in L]
    elif kind == "line":
        mult = small_multiples(some_point())
        L = [mult[rnd.choice((-1, 1)) * rnd.randrange(1, 9)] for _ in range(k)]
        R = [mult[rnd.choice((-1, 1)) * rnd.randrange(1, 9)] for _ in range(k)]
    else:
        assert kind is None
        R = [some_point() for _ in range(k)]
    L, R = b"".join(L), b"".join(R)
    ch, state = cases.replay(n, L, R)
    exp = cases.expect_P(n, Q, Gf, Hf, G, H, L, R, a, b, ch)
    P = L[:64] if p_is_l0 else exp
    shifted = o.point_add(P, o.generator())

    def verdict(pt):
        return 1 if o.ipp_verify(cases.LABEL, n, Gf, Hf, pt, Q, G, H, L, R, a, b) == 0 else 0
    return dict(n=n, kind=kind, Q=Q, w=w, Gf=Gf, Hf=Hf, G=G, H=H, L=L, R=R, ab=a + b, ch=ch, state=state, expect=exp, P=P,
                P_shifted=shifted, bit=verdict(P), bit_shifted=verdict(shifted))


def ipp_batch(n, nb):
    """nb proofs of length n: honest, twin, opposite and line in turn; the second proof has P := L_0"""
    kinds = (None, "twin", "opposite", "line")
    return [ipp_case(n, 900 + 13 * n + p, kinds[p % 4], p_is_l0=(p == 1)) for p in range(nb)]
