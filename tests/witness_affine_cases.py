"""Affine chains of bpgpu_witness gate programs (include/bpgpu.h "affine member"): pass 2 of the recognition restated on the Program of
tests/witness_cases.py on top of pass 1 as tests/witness_chain_cases.py restates it -- the extended chains, their affine members and
the extended compressed levels -- and programs made to put every boundary of k_witness_scan<true> (256 threads, runs of
ceil(M / 256) elements) under an affine chain.  The reference of every test stays Program.evaluate on Python integers, computed once
per case.  No GPU."""
import random

import witness_cases as wc
import witness_chain_cases as cc

pm = wc.pm
N = wc.N
L, R, O, V, ONE = wc.L, wc.R, wc.O, wc.V, wc.ONE
CHAIN_MS = (1, 2, 255, 256, 257, 513)
SEGMENTS = cc.SEGMENTS
LONG = cc.LONG
ELEM_START, ELEM_RIGHT, ELEM_AFFINE = cc.ELEM_START, cc.ELEM_RIGHT, 1 << 27      # WIT_ELEM_* of csrc/kernels.h
FIELDS = ("chains1", "chains2", "members1", "members2", "affine1", "affine2", "longest1", "longest2", "levels1", "levels2")
_nz, _any, _free, _provers = cc._nz, cc._any, cc._free, cc._provers


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def analyse(prog):
    """-> (pred, link_right, affine, extended compressed level per gate, figures): pass 1 is cc's; pass 2 runs in program order over
    the MUL gates it left without a predecessor.  figures = {"chains": (phase 1, phase 2), "members": .., "affine": .., "longest": ..,
    "levels": ..}, all on the extended chains"""
    n, n1 = prog.n, prog.phase1
    pred, right = (list(x) for x in cc._analyse(prog)[:2])
    succ = {j: i for i, j in enumerate(pred) if j is not None}          # every product member is known before pass 2 starts
    affine, level, head, length = [False] * n, [0] * n, [None] * n, {}
    chains, members, naff, longest, levels = [0, 0], [0, 0], [0, 0], [0, 0], [0, 0]
    for i, (op, _, left, rght) in enumerate(prog.gates):
        ph = int(i >= n1)
        lo = n1 if ph else 0
        rows = (cc._stored(prog, left), cc._stored(prog, rght))
        on_phase = [[(kind, idx) for kind, idx in row if kind <= O and idx >= lo] for row in rows]
        if op == wc.MUL and pred[i] is None:
            for side in (0, 1):
                link = on_phase[side]
                if len(link) != 1 or link[0][0] != O or link[0][1] in succ or on_phase[1 - side]:
                    continue
                pred[i], right[i], affine[i] = link[0][1], bool(side), True
                succ[pred[i]] = i
                naff[ph] += 1
                break
        if pred[i] is not None:
            j = pred[i]
            head[i] = j if pred[j] is None else head[j]
            chains[ph] += head[i] == j
            members[ph] += 1
            length[head[i]] = length.get(head[i], 0) + 1
            longest[ph] = max(longest[ph], length[head[i]])
            level[i] = level[j]
        else:
            reads = [idx for row in on_phase for _, idx in row]
            level[i] = 0 if op == wc.INPUT or not reads else 1 + max(level[r] for r in reads)
        levels[ph] = max(levels[ph], level[i] + 1)
    figs = {"chains": tuple(chains), "members": tuple(members), "affine": tuple(naff), "longest": tuple(longest), "levels": tuple(levels)}
    return pred, right, affine, level, figs


def figures(prog):
    """the ten fields of bpgpu_witness_affine_chains"""
    f = analyse(prog)[4]
    return {k + str(ph + 1): f[k][ph] for k in ("chains", "members", "affine", "longest", "levels") for ph in (0, 1)}


def scan_lists(prog):
    """what the scan form walks on the extended chains: per extended compressed level (phase 1's first) the ordinary gates in program
    order and the element words of the chains headed there, chain after chain"""
    pred, right, affine, level, f = analyse(prog)
    succ = {j: i for i, j in enumerate(pred) if j is not None}
    out = [([], []) for _ in range(sum(f["levels"]))]
    for i in range(prog.n):
        if pred[i] is not None:
            continue
        gates, elems = out[(f["levels"][0] if i >= prog.phase1 else 0) + level[i]]
        gates.append(i)
        e, first = succ.get(i), ELEM_START
        while e is not None:
            elems.append(e | first | (ELEM_RIGHT if right[e] else 0) | (ELEM_AFFINE if affine[e] else 0))
            e, first = succ.get(e), 0
    return out


def library_copy(prog):
    """the program as the library keeps its rows: the link term of an affine member first in its link row (the sums are exact)"""
    pred, right, affine = analyse(prog)[:3]
    out = wc.Program(prog.m, prog.nchi)
    out.n1 = prog.n1
    for i, (op, arg, left, rght) in enumerate(prog.gates):
        rows = [list(left), list(rght)]
        if affine[i]:
            lo = prog.phase1 if i >= prog.phase1 else 0
            row = rows[int(right[i])]
            at = next(t for t, (kind, idx, _) in enumerate(row) if kind <= O and idx >= lo)
            row.insert(0, row.pop(at))
        out.gates.append((op, arg, rows[0], rows[1]))
    return out


# ---- the programs ------------------------------------------------------------------------------------------------------------------
def _rest(rnd, prog, param, k):
    """what an affine link row holds beside its link term: terms that read nothing of the phase, now one, now three, some with chi
    parts"""
    c = (_nz(rnd), _nz(rnd)) + (None,) * (prog.nchi - 1) if param and k % 4 == 2 else _nz(rnd)
    rest = [(V, rnd.randrange(prog.m), c)]
    if k % 3 == 1:
        rest += [(ONE, 0, _any(rnd)), (V, rnd.randrange(prog.m), _nz(rnd))]
    return rest


def _affine_chain(rnd, prog, head, count, param, product_every=0, long_free_at=None):
    """`count` members on `head`, the link now left, now right and anywhere in its row; in a parametric phase some link coefficients
    are stored in the chi block alone and some free rows carry chi parts; product_every: every such member is a pure product"""
    last = head
    for k in range(count):
        coeff = (None, _nz(rnd)) + (None,) * (prog.nchi - 1) if param and k % 7 == 3 else _nz(rnd)
        link = [(O, last, coeff)]
        if not (product_every and k % product_every == product_every - 1):
            rest = _rest(rnd, prog, param, k)
            at = k % (len(rest) + 1)
            link = rest[:at] + link + rest[at:]
        free = _free(rnd, prog, param and k % 5 == 1)
        if k == long_free_at:
            free = [(V, t % prog.m, _nz(rnd)) for t in range(256)] + [(ONE, 0, 1)]          # 257 terms: above rows_lane_max()
        last = prog.mul(link, free) if k % 3 else prog.mul(free, link)
    return last


def _horner_gates(prog, k, base):
    """Horner evaluation of the committed values base .. base + k and base + k .. base + 2 k at the challenge z: k - 1 multipliers a
    side (the last sum, o + x_0, is the constraint's)"""
    z = (ONE, 0, (None, 1))
    for side in (base, base + k):
        last = prog.mul([(V, side + k - 1, 1)], [z])
        for i in range(k - 2, 0, -1):
            last = prog.mul([(O, last, 1), (V, side + i, 1)], [z])


def horner_gadget(cs, x, y):
    """two committed vectors are equal under a random linear combination, against the model's constraint system (oracle/pymodel.py)"""
    k = len(x)

    def cb(cs):
        z = cs.challenge_scalar(wc.SHUFFLE_LABEL)
        accs = []
        for side in (x, y):
            acc = pm.lc_var(side[k - 1])
            for i in range(k - 2, -1, -1):
                _, _, o = cs.multiply(acc, pm.lc_const(z))
                acc = pm.lc_add(pm.lc_var(o), pm.lc_var(side[i]))
            accs.append(acc)
        cs.constrain(pm.lc_sub(accs[0], accs[1]))
    cs.specify_randomized_constraints(cb)


_horners = {}


def horner_case(k):
    """n = 2 (k - 1) gates in phase 2, k - 1 uncompressed levels, two affine chains of k - 2 members (built once per k)"""
    if k in _horners:
        return _horners[k]
    prog = wc.Program(2 * k, nchi=1)
    prog.end_phase1()
    _horner_gates(prog, k, 0)
    rnd = random.Random(70 + k)
    provers = []
    for chi in wc.CHIS + (rnd.randrange(N), rnd.randrange(N)):
        xs = [rnd.randrange(N) for _ in range(k)]
        provers.append((xs + xs, (), (chi,)))

    def gadget(cs, var, v, inputs):
        horner_gadget(cs, var[:k], var[k:])
    _horners[k] = wc.Case("horner%d" % k, prog, provers, gadget, breaker=lambda v, inputs: ([(v[0] + 1) % N] + list(v[1:]), inputs))
    return _horners[k]


def horner_circuit(constraints, q1, nchi=1):
    """(q, nchi, row_ptr, kind, idx, coeff) of the Horner gadget's constraints: a `One` term of a second-phase constraint is the
    multiplier's right operand z itself, stored as 1 in the chi block (wc.circuit_from is written for the shuffle's -z)"""
    import mpc_dealer as md
    rows = [[(var, (None, 1) if r >= q1 and var == pm.ONE else c) for var, c in lc.items()] for r, lc in enumerate(constraints)]
    rp, kd, ix, cf, _ = md.circuit_rows(rows, nchi=nchi)
    return len(rows), nchi, rp, kd, ix, cf


def chain_case(count):
    """one affine chain of `count` members in phase 2: the run length changes at 256 / 257 members; member 1 (where there is one) has a
    free row of 257 terms"""
    rnd = random.Random(19000 + count)
    prog = wc.Program(5, nchi=1)
    prog.end_phase1()
    head = prog.mul([(V, 0, 1), (ONE, 0, (None, N - 1))], [(V, 1, _nz(rnd))])
    _affine_chain(rnd, prog, head, count, True, long_free_at=1)
    return wc.Case("affine%d" % count, prog, _provers(rnd, prog))


def segments_case():
    """chains of 1, 3, 256, 2 and 300 members at one level, the kinds alternating: pure products, affine, pure products, .."""
    rnd = random.Random(1562)
    prog = wc.Program(6)
    for s, count in enumerate(SEGMENTS):
        head = prog.mul([(V, rnd.randrange(6), _nz(rnd))], [(V, rnd.randrange(6), 1), (ONE, 0, _nz(rnd))])
        if s % 2:
            _affine_chain(rnd, prog, head, count, False)
        else:
            cc._chain(rnd, prog, head, count, False)
    prog.end_phase1()
    return wc.Case("affsegments", prog, _provers(rnd, prog))


def long_case():
    """two chains of 4 099 affine members: 32.02 elements per thread"""
    rnd = random.Random(LONG + 1)
    prog = wc.Program(8, nchi=1)
    prog.end_phase1()
    for _ in range(2):
        head = prog.mul([(V, 0, 1), (ONE, 0, (None, N - 1))], [(V, 1, 1), (ONE, 0, (None, N - 1))])
        _affine_chain(rnd, prog, head, LONG, True)
    return wc.Case("afflong2x%d" % LONG, prog, _provers(rnd, prog, 3))


def mixed_case():
    """everything around an affine chain that the recognition and the kernel must get right (see the test that reads the marks)"""
    rnd = random.Random(177)
    prog = wc.Program(4, nchi=2)
    g0 = prog.mul([(V, 0, 1), (ONE, 0, 5)], [(V, 1, 1)])
    g1 = prog.mul([(R, g0, 1), (ONE, 0, 1)], [(O, g0, N - 1), (V, 2, 1)])                 # a head at level 1
    # chain A on g1 mixes the kinds: product, affine, affine with a free row that is 0 whatever the values (the rest of A is then B
    # alone), affine, product, affine with an explicit zero link coefficient (its a_O is f g), affine
    a1 = prog.mul([(O, g1, _nz(rnd))], _free(rnd, prog, False))
    a2 = prog.mul(_free(rnd, prog, False), [(V, 0, _nz(rnd)), (O, a1, 1 << 251)])
    a3 = prog.mul([(O, a2, _nz(rnd)), (V, 1, 3)], [(V, 3, 1), (V, 3, N - 1)])
    a4 = prog.mul([(ONE, 0, 7), (O, a3, N - 1), (V, 2, 1)], _free(rnd, prog, False))
    a5 = prog.mul(_free(rnd, prog, False), [(O, a4, _nz(rnd))])
    a6 = prog.mul([(O, a5, 0), (V, 1, 1)], _free(rnd, prog, False))
    a7 = prog.mul(_free(rnd, prog, False), [(V, 2, N - 1), (O, a6, (N + 1) // 2)])
    # a pure-product gate and an affine gate competing for one a_O, in either order: the product gate is the member
    p1 = prog.mul([(O, g0, 1), (V, 0, 1)], [(V, 1, 1)])              # affine on g0, comes first, loses
    p2 = prog.mul([(O, g0, 1)], [(V, 2, 1)])                          # product on g0: the member
    q0 = prog.mul([(V, 1, 1)], [(V, 2, 1), (ONE, 0, 1)])
    q1 = prog.mul([(O, q0, 2)], [(V, 3, 1)])                          # product on q0: the member
    q2 = prog.mul([(V, 3, 1)], [(O, q0, 1), (ONE, 0, 1)])             # affine on q0, comes second, loses
    # two gates affine-linking to one a_O: the first is the member, the second an ordinary gate and a head of its own
    d0 = prog.mul([(V, 0, 1)], [(V, 3, 1)])
    d1 = prog.mul([(O, d0, 1), (V, 0, 1)], [(V, 0, 1)])
    d2 = prog.mul([(O, d0, 1), (V, 1, 1)], [(V, 1, 1)])
    d3 = prog.mul([(V, 1, 1)], [(ONE, 0, 1), (O, d2, N - 1)])
    # a gate that pass 1 called a head (of the product member h2) and pass 2 makes a member of d3's chain
    h1 = prog.mul([(O, d3, 3), (V, 2, 1)], [(V, 0, 1)])
    h2 = prog.mul([(O, h1, 1)], [(V, 1, 1), (ONE, 0, 1)])
    # what stays ordinary: both rows read the phase; a link through a_L; an ordinary gate reading mid-chain members
    s1 = prog.mul([(O, a7, 1), (V, 0, 1)], [(O, a7, 1)])
    s2 = prog.mul([(L, a2, 1), (V, 0, 1)], [(V, 1, 1)])
    x1 = prog.mul([(L, a3, 1), (R, a4, 1)], [(O, a6, 1), (L, a7, 1)])
    prog.end_phase1()
    # phase 2: link coefficients stored in a chi block alone, free rows and link rows that read phase 1, and a link coefficient split
    # over two blocks, which stays ordinary
    h = prog.mul([(V, 0, (1, None, N - 1))], [(O, g1, 1), (ONE, 0, 1)])
    e1 = prog.mul([(O, h, (None, 7, None)), (O, a7, 1)], [(L, a1, 1), (V, 1, (None, None, 1))])
    e2 = prog.mul([(R, a2, 1), (ONE, 0, (None, N - 1, None))], [(V, 1, (3, 1, None)), (O, e1, (None, None, N - 1))])
    e3 = prog.mul([(O, e2, (1 << 251, None, None)), (L, x1, 1), (ONE, 0, (None, None, 5))], [(O, x1, 1), (V, 2, 1)])
    e4 = prog.mul([(O, e3, (2, 3, None)), (V, 0, 1)], _free(rnd, prog, True))
    y1 = prog.mul([(L, e2, 1), (R, e3, 1)], [(O, e4, 1), (O, e1, 1)])
    provers = []
    for chi in ((0, 0), (1, N - 1), (rnd.randrange(N), rnd.randrange(N)), (N - 1, 1)):
        provers.append(([rnd.randrange(1, N) for _ in range(4)], (), chi))
    case = wc.Case("affmixed", prog, provers[::-1])
    case.mark = dict(g0=g0, g1=g1, a=(a1, a2, a3, a4, a5, a6, a7), p=(p1, p2), q=(q0, q1, q2), d=(d0, d1, d2, d3), h12=(h1, h2),
                     s=(s1, s2), x1=x1, h=h, e=(e1, e2, e3, e4), y1=y1)
    return case


def lazy_case(count=300):
    """one affine chain in which every A = c g and every B = f g is lazily n - 1 (tests/lazy_sum_cases.py: a product of plain value
    -2^-261 has the Montgomery residue n - 1, the heaviest operand a product can be handed): g is one such product, c = 1, and f is
    the canonical 1; the head's a_O is one as well"""
    import lazy_sum_cases as lz
    rnd = random.Random(1261)
    vals = [rnd.randrange(1, N) for _ in range(3)]
    prog = wc.Program(3)
    last = prog.mul([(V, 0, lz.C * lz.inv(vals[0]) % N)], [(V, 1, lz.inv(vals[1]))])
    for k in range(count):
        free = [(V, k % 3, lz.C * lz.inv(vals[k % 3]) % N)]
        link = [(O, last, 1), (ONE, 0, 1)] if k % 4 else [(ONE, 0, 1), (O, last, 1)]
        last = prog.mul(link, free) if k % 2 else prog.mul(free, link)
    prog.end_phase1()
    return wc.Case("afflazy%d" % count, prog, [(vals, (), ())])


_cases = None


def cases():
    """every new program that is evaluated, built once"""
    global _cases
    if _cases is None:
        _cases = ([chain_case(m) for m in CHAIN_MS] + [segments_case(), mixed_case(), lazy_case(), horner_case(9), horner_case(300),
                                                       long_case()])
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)
