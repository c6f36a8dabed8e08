"""Product chains of bpgpu_witness gate programs (include/bpgpu.h "product chains"): the definition restated on the Program of
tests/witness_cases.py -- members, heads, the longest chain and the compressed levels per phase -- and programs made to put every
boundary of the scan form (csrc/k_witness.hip k_witness_scan: 256 threads, a run of ceil(M / 256) elements each) under a chain.  The
reference of every test stays Program.evaluate on Python integers, computed once per case.  No GPU."""
import random

import witness_cases as wc

N = wc.N
L, R, O, V, ONE = wc.L, wc.R, wc.O, wc.V, wc.ONE
CHAIN_MS = (1, 2, 255, 256, 257, 511, 513)
SEGMENTS = (1, 3, 256, 2, 300)
LONG = 4099


def _stored(prog, row):
    """(kind, idx) of every stored term of a row, over all blocks"""
    return [(kind, idx) for kind, idx, coeff in row for part in prog.parts(coeff) if part is not None]


def _analyse(prog):
    """-> (pred, link_right, compressed level per gate, figures)"""
    n, n1 = prog.n, prog.phase1
    pred, right, succ, level, head = [None] * n, [False] * n, [None] * n, [0] * n, [None] * n
    length = {}
    chains, members, longest, levels = [0, 0], [0, 0], [0, 0], [0, 0]
    for i, (op, _, left, rght) in enumerate(prog.gates):
        ph = int(i >= n1)
        lo = n1 if ph else 0
        rows = (_stored(prog, left), _stored(prog, rght))
        reads = [idx for row in rows for kind, idx in row if kind <= O and idx >= lo]
        level[i] = 0 if op == wc.INPUT or not reads else 1 + max(level[r] for r in reads)
        if op == wc.MUL:
            for side in (0, 1):
                link, free = rows[side], rows[1 - side]
                if len(link) != 1 or link[0][0] != O or link[0][1] < lo or succ[link[0][1]] is not None:
                    continue
                if any(kind <= O and idx >= lo for kind, idx in free):
                    continue
                j = link[0][1]
                pred[i], right[i], succ[j] = j, bool(side), i
                head[i] = j if pred[j] is None else head[j]
                if head[i] == j:
                    chains[ph] += 1
                members[ph] += 1
                length[head[i]] = length.get(head[i], 0) + 1
                longest[ph] = max(longest[ph], length[head[i]])
                level[i] = level[j]
                break
        levels[ph] = max(levels[ph], level[i] + 1)
    return pred, right, level, {"chains": tuple(chains), "members": tuple(members), "longest": tuple(longest), "levels": tuple(levels)}


def analyse(prog):
    """-> (pred, link_right, figures): per gate its predecessor (None: an ordinary gate) and whether its link is the right row;
    figures = {"chains": (phase 1, phase 2), "members": .., "longest": .., "levels": ..} -- levels the compressed ones"""
    pred, right, _, figs = _analyse(prog)
    return pred, right, figs


ELEM_START, ELEM_RIGHT = 1 << 25, 1 << 26        # WIT_ELEM_* of csrc/kernels.h


def scan_lists(prog):
    """what the scan form walks, from the restated definition: per compressed level (phase 1's first) the ordinary gates in program
    order and the element words of the chains headed there, chain after chain"""
    pred, right, level, f = _analyse(prog)
    succ = {j: i for i, j in enumerate(pred) if j is not None}
    out = [([], []) for _ in range(sum(f["levels"]))]
    for i in range(prog.n):
        if pred[i] is not None:
            continue
        gates, elems = out[(f["levels"][0] if i >= prog.phase1 else 0) + level[i]]
        gates.append(i)
        e, first = succ.get(i), ELEM_START
        while e is not None:
            elems.append(e | first | (ELEM_RIGHT if right[e] else 0))
            e, first = succ.get(e), 0
    return out


def figures(prog):
    """the eight fields of bpgpu_witness_chains"""
    f = analyse(prog)[2]
    return {k + str(ph + 1): f[k][ph] for k in ("chains", "members", "longest", "levels") for ph in (0, 1)}


def parent_plan(prog, nb):
    """bpgpu_witness_plan as the library gave it before there was a scan form: the helper's levels, and the width rule"""
    l1, l2, widest, long_rows = prog.levels()

    def route(gates, levels):
        rounds = (nb + 1023) // 1024
        if not gates:
            return 0
        if rounds > gates:
            return 1
        return 2 if gates >= 2 * max(rounds, 1) * levels else 1
    return {"levels1": l1, "levels2": l2, "widest": widest, "long_rows": long_rows, "inputs": prog.ninp,
            "route1": route(prog.phase1, l1), "route2": route(prog.n - prog.phase1, l2)}


# ---- the programs ------------------------------------------------------------------------------------------------------------------
def _nz(rnd):
    return rnd.choice(wc.EDGE[1:] + (rnd.randrange(1, N),))


def _any(rnd):
    return rnd.choice(wc.EDGE + (rnd.randrange(N),))


def _free(rnd, prog, chi_part):
    """a free row: two committed values and the constant, so that it rarely vanishes"""
    c = (_nz(rnd), _nz(rnd)) + (None,) * (prog.nchi - 1) if chi_part else _nz(rnd)
    return [(V, rnd.randrange(prog.m), _nz(rnd)), (V, rnd.randrange(prog.m), c), (ONE, 0, _any(rnd))]


def _chain(rnd, prog, head, count, param):
    """`count` members on `head`, the link now left, now right; in a parametric phase some link coefficients are stored in the chi
    block (a link row is ONE stored term: a constant part beside it would make two)"""
    last = head
    for k in range(count):
        coeff = (None, _nz(rnd)) if param and k % 7 == 3 else _nz(rnd)
        link, free = [(O, last, coeff)], _free(rnd, prog, param and k % 5 == 1)
        last = prog.mul(link, free) if k % 3 else prog.mul(free, link)
    return last


def _provers(rnd, prog, count=4):
    """prover 0 (the one a batch of one runs): random non-zero values and a random challenge, so that no factor vanishes; the others
    draw from the edges of the field, chi = 0, 1, n - 1 in turn (chi = 0 zeroes a coefficient that has a chi part alone)"""
    out = []
    for p in range(count):
        chi = tuple(((rnd.randrange(1, N),) + wc.CHIS)[(p + j) % 4] for j in range(prog.nchi))
        out.append(([_any(rnd) if p else rnd.randrange(1, N) for _ in range(prog.m)],
                    [(_any(rnd), _any(rnd)) for _ in range(prog.ninp)], chi))
    return out


def chain_case(count):
    """one chain of `count` members in phase 2: the run length changes at 256 / 257 members, and the last thread's run is ragged"""
    rnd = random.Random(9000 + count)
    prog = wc.Program(5, nchi=1)
    prog.end_phase1()
    head = prog.mul([(V, 0, 1), (ONE, 0, (None, N - 1))], [(V, 1, _nz(rnd))])
    _chain(rnd, prog, head, count, True)
    return wc.Case("chain%d" % count, prog, _provers(rnd, prog))


def segments_case():
    """chains of 1, 3, 256, 2 and 300 members at one level (562 elements, runs of 3): segments start at a run's start, inside runs and
    in other waves than their heads' neighbours; the 256- and the 300-chain each cross a wave"""
    rnd = random.Random(562)
    prog = wc.Program(6)
    for count in SEGMENTS:
        head = prog.mul([(V, rnd.randrange(6), _nz(rnd))], [(V, rnd.randrange(6), 1), (ONE, 0, _nz(rnd))])
        _chain(rnd, prog, head, count, False)
    prog.end_phase1()
    return wc.Case("segments", prog, _provers(rnd, prog))


def long_case():
    """two chains of 4 099 members: 32.02 elements per thread"""
    rnd = random.Random(LONG)
    prog = wc.Program(8, nchi=1)
    prog.end_phase1()
    for _ in range(2):
        head = prog.mul([(V, 0, 1), (ONE, 0, (None, N - 1))], [(V, 1, 1), (ONE, 0, (None, N - 1))])
        _chain(rnd, prog, head, LONG, True)
    return wc.Case("long2x%d" % LONG, prog, _provers(rnd, prog, 3))


def mixed_case():
    """everything around a chain that the recognition and the kernel must get right (see the test that reads MIXED)"""
    rnd = random.Random(77)
    prog = wc.Program(4, nchi=2)
    mark = {}
    g_in = prog.input()                                                    # heads that are INPUT and BIT gates
    g_bit = prog.bit([(V, 0, 1)], 3)
    g2 = prog.mul([(V, 0, 1), (ONE, 0, 5)], [(V, 1, 1)])
    g3 = prog.mul([(O, g2, 1), (V, 1, 1)], [(L, g2, 1)])                   # two terms: no link
    g4 = prog.mul([(R, g3, 1), (ONE, 0, 1)], [(O, g3, N - 1), (V, 2, 1)])  # a head at level 2 that reads other gates
    # chain A on g4: N - 1 on the left, 2^251 on the right, then a free row that is 0 whatever the values: the rest of A is 0
    a1 = prog.mul([(O, g4, N - 1)], _free(rnd, prog, False))
    a2 = prog.mul(_free(rnd, prog, False), [(O, a1, 1 << 251)])
    a3 = prog.mul([(O, a2, _nz(rnd))], [(V, 3, 1), (V, 3, N - 1)])
    a4 = prog.mul(_free(rnd, prog, False), [(O, a3, 1)])
    a5 = prog.mul([(O, a4, 1)], _free(rnd, prog, False))
    # chain B on the INPUT gate: a free row of 257 terms
    b1 = prog.mul([(O, g_in, _nz(rnd))], _free(rnd, prog, False))
    b2 = prog.mul([(V, k % 4, _nz(rnd)) for k in range(256)] + [(ONE, 0, 1)], [(O, b1, 1)])
    b3 = prog.mul([(O, b2, (N + 1) // 2)], _free(rnd, prog, False))
    # chain C on the BIT gate: an explicit zero coefficient is still a term, and zeroes what follows
    c1 = prog.mul([(O, g_bit, _nz(rnd))], _free(rnd, prog, False))
    c2 = prog.mul([(O, c1, 0)], _free(rnd, prog, False))
    c3 = prog.mul(_free(rnd, prog, False), [(O, c2, 1)])
    # two gates linking to one a_O: the first is the member, the second an ordinary gate -- and the head of a chain of its own
    d1 = prog.mul([(O, g2, 1)], [(V, 0, 1)])
    d2 = prog.mul([(O, g2, 1)], [(V, 1, 1)])
    d3 = prog.mul([(V, 1, 1)], [(O, d2, N - 1)])
    # an ordinary gate on the next level reading a_L, a_R and a_O of mid-chain members; one whose rows are both single a_O terms
    x1 = prog.mul([(L, a2, 1), (R, a2, 1)], [(O, a1, 1), (L, b2, 1), (R, b2, 1)])
    x2 = prog.mul([(O, a5, 1)], [(O, c3, 1)])
    prog.end_phase1()
    # phase 2: the head reads phase-1 multipliers only (level 0); coefficients stored only in a chi block; free rows over phase 1
    h = prog.mul([(V, 0, (1, None, N - 1))], [(O, g4, 1), (ONE, 0, 1)])
    e1 = prog.mul([(O, h, (None, 7, None))], [(L, a1, 1), (V, 1, (None, None, 1))])
    e2 = prog.mul([(R, b2, 1), (ONE, 0, (None, N - 1, None))], [(O, e1, (None, None, N - 1))])
    e3 = prog.mul([(O, e2, (1 << 251, None, None))], [(O, x1, 1), (V, 2, 1)])
    e4 = prog.mul([(O, e3, N - 1)], _free(rnd, prog, True))
    y1 = prog.mul([(L, e2, 1), (R, e3, 1)], [(O, e4, 1), (O, e1, 1)])
    mark.update(g_in=g_in, g_bit=g_bit, g2=g2, g3=g3, g4=g4, a=(a1, a2, a3, a4, a5), b=(b1, b2, b3), c=(c1, c2, c3), d=(d1, d2, d3),
                x=(x1, x2), h=h, e=(e1, e2, e3, e4), y1=y1)
    provers = []
    for chi in ((0, 0), (1, N - 1), (rnd.randrange(N), rnd.randrange(N)), (N - 1, 1)):
        provers.append(([rnd.randrange(1, N) for _ in range(4)], [(rnd.randrange(1, N), _nz(rnd))], chi))
    case = wc.Case("mixed", prog, provers[::-1])
    case.mark = mark
    return case


def lazy_chain_case(count=300):
    """one chain in which every factor f = c r is lazily n - 1 (tests/lazy_sum_cases.py: a product of plain value -2^-261 has the
    Montgomery residue n - 1, the heaviest operand the next product can be handed): the free row is one such product, the link
    coefficient 1, and the head's a_O is one as well"""
    import lazy_sum_cases as lz
    rnd = random.Random(261)
    vals = [rnd.randrange(1, N) for _ in range(3)]
    prog = wc.Program(3)
    last = prog.mul([(V, 0, lz.C * lz.inv(vals[0]) % N)], [(V, 1, lz.inv(vals[1]))])
    for k in range(count):
        free = [(V, k % 3, lz.C * lz.inv(vals[k % 3]) % N)]
        link = [(O, last, 1)]
        last = prog.mul(link, free) if k % 2 else prog.mul(free, link)
    prog.end_phase1()
    return wc.Case("lazychain%d" % count, prog, [(vals, (), ())])


_cases = None


def cases():
    """every new program that is evaluated, built once"""
    global _cases
    if _cases is None:
        _cases = [chain_case(m) for m in CHAIN_MS] + [segments_case(), mixed_case(), long_case()]
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


_shuffles = {}


def shuffle(k):
    """wc.shuffle_case(k) for the plan and chain figures (k = 300 also for the constraint check), built once"""
    if k not in _shuffles:
        _shuffles[k] = wc.shuffle_case(k)
    return _shuffles[k]
