"""Inner-product prover sessions over generators, vectors and challenges chosen so that the rounds' point additions meet the exact
cases of the group law, and a CPU shadow of who adds what to whom.  Test infrastructure, no GPU: tests/test_ipp_round_cases.py
checks it, tests/test_gpu_ipp_round_cases.py drives bpgpu_ipp_begin, _begin_gens, _round, _fold, _finish, _folded_gens and _run_fs
with it.

Every generator is a known multiple k_i B of the curve generator B (k_i = 0: the identity), so every point the prover computes is
(sum s_i k_i) B: an integer mod n here, one scalar multiplication of the oracle where bytes are compared.  `rounds` is the prover
(inner_product_proof.rs:87-184) on these integers; it never touches the library under test.

The shadow walks the kernels' addition orders on those integers and reports, per site,

  dbl       acc == addend
  cancel    acc == -addend
  ident     an identity operand: an accumulator that HAS held a point and lost it, an identity partial sum, an identity input point
  zero_out  the site's result is the identity (64 zero bytes at the boundary)

Sites and the code they mirror:
  lane      a lane accumulator of k_fixed_msm_ipp<C, 128> (pairs lo + l, lo + l + 128, ...) or k_fixed_msm_ipp_g<C> (pair-lanes,
            stride 8) over the compact terms B, n0/2 G terms, n0/2 H terms (k_ipp_gens_scalars; hi/lo enumeration for cur < n0)
  reduce    block_sum<128> (lanes tid, tid + s for s = 64 .. 1) or the grouped kernel's shuffle butterfly (offsets 8, 16, 32: bits
            0, 1, 2 of the pair-lane)
  partials  the chunk partial sums: k_segmented_sum<16> (a strided pass, block_sum<16>) after bpgpu_ipp_round, k_ipp_round_tail's
            strided pass of 16 lanes and butterfly at offsets 8, 4, 2, 1 inside bpgpu_ipp_run_fs
  norm_run  k_batch_normalize<8>: lane r normalises the points 8 r .. 8 r + 7 of the flat index p h + i of the folded generators
  fold_lane straus_body<2>: lane p h + i computes s0 G_L[i] + s1 G_R[i], 64 signed 4-bit windows from the top, 4 doublings between
            them, the left point first; 64 lanes to a wave, `pinf` per lane, `skip` where a whole wave's j-th points are identities

Launch shapes the cases rely on (fixed_msm_ipp_chunks / launch_fixed_ipp; LAUNCHES below, asserted by test_ipp_round_cases.py):
  c = 8, n0 = 16:  nb = 3 -> block kernel, 2 chunks of 272 pairs;  nb = 8, 9 -> grouped kernel, 3 chunks of 184 pairs
  c = 8, n0 = 128, nb = 8 -> grouped kernel, 4 128 pairs in 17 chunks of 248: the tail's strided pass iterates twice
  c = 16, n0 = 16: nb = 3 -> block kernel, 1 chunk;  nb = 8 -> grouped kernel, 2 chunks of 136 pairs

Event counts of the committed cases (test_ipp_round_cases.py asserts every entry is non-zero; `python tests/ipp_round_cases.py`
prints them):
  block kernel (c = 8, nb = 3):    lane dbl 16 cancel 6 ident 3; reduce dbl 4 cancel 6; partials dbl 4 cancel 3; zero_out 5
  grouped kernel (c = 8, nb = 8):  lane dbl 21 cancel 9 ident 5; reduce dbl 3 cancel 3; partials dbl 4 cancel 3; zero_out 8
  (`ident` at reduce and partials: hundreds, a sparse sum is mostly identity operands; of them 16 and 61 are identity PARTIAL sums
  in k_segmented_sum's strided pass, where a lane's first addition does not count its own empty accumulator)
  tail at 2 chunks:                dbl 4 cancel 3 ident 540 (identity partials 20) zero_out 7
  tail at 3 chunks:                dbl 4 cancel 3 ident 751 (identity partials 67) zero_out 10
  tail at 17 chunks:               dbl 4 cancel 4 ident 235 (identity partials 120) zero_out 5; the equal pair at chunks (0, 16) meets in lane 0's strided
                                   pass, second iteration, and the pair at (3, 11) in the butterfly at offset 8
  fold lanes (A.2, A.3):           dbl 4 cancel 120 ident (pinf) 258 zero_out 9, and a wave with `skip` on either side
  normalisation runs (A.1):        identities first, middle and last in a run, a whole run next to a partial one, the short run
"""
import functools
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

import oracle_lib as o
import window_digits as wd

N = o.N
ZERO = bytes(64)
LABEL = b"innerproducttest"
EVENTS = ("dbl", "cancel", "ident", "zero_out")


def inv(x):
    assert x % N
    return pow(x, N - 2, N)


_PT = {}


def pt(d):
    """d B as 64 bytes"""
    d %= N
    if d == 0:
        return ZERO
    if d not in _PT:
        _PT[d] = o.point_mul(o.s2b(d), o.generator())
    return _PT[d]


def pts(ds):
    return b"".join(pt(d) for d in ds)


def dot(x, y):
    return sum(p * q for p, q in zip(x, y)) % N


# ------------------------------------------------------------------ the prover on discrete logarithms
class Case:
    """one session: nb proofs of length n.  kG, kH: per proof the generators' logarithms (shared: ONE list); q: Q's; gf, hf, a, b per
    proof; us[r][p]: the challenge of round r (stepwise calls only).  resident sessions: kB, w (Q = w B, so q = w kB) and c."""

    def __init__(self, name, n, nb, kG, kH, q, gf, hf, a, b, us, shared=False, **kw):
        self.name, self.n, self.nb, self.shared = name, n, nb, shared
        self.kG, self.kH, self.q, self.gf, self.hf, self.a, self.b, self.us = kG, kH, q, gf, hf, a, b, us
        self.__dict__.update(kw)

    def gens_of(self, p):
        return (self.kG, self.kH) if self.shared else (self.kG[p], self.kH[p])

    def flat(self, rows):
        return o.scalars([v for r in rows for v in r])


def rounds(case, p):
    """proof p of `case` -> ([(L, R, g, h)] per round, a, b): L, R and the generators AFTER the round's fold as logarithms, the final
    a and b"""
    kG, kH = case.gens_of(p)
    n = case.n
    g = [k * f % N for k, f in zip(kG, case.gf[p])]
    hh = [k * f % N for k, f in zip(kH, case.hf[p])]
    a, b, q = list(case.a[p]), list(case.b[p]), case.q[p]
    out = []
    r = 0
    while n > 1:
        h = n // 2
        cL, cR = dot(a[:h], b[h:]), dot(a[h:], b[:h])
        L = (dot(a[:h], g[h:]) + dot(b[h:], hh[:h]) + cL * q) % N
        R = (dot(a[h:], g[:h]) + dot(b[:h], hh[h:]) + cR * q) % N
        u = case.us[r][p]
        ui = inv(u)
        g = [(ui * g[i] + u * g[h + i]) % N for i in range(h)]
        hh = [(u * hh[i] + ui * hh[h + i]) % N for i in range(h)]
        a = [(a[i] * u + a[h + i] * ui) % N for i in range(h)]
        b = [(b[i] * ui + b[h + i] * u) % N for i in range(h)]
        out.append((L, R, g, hh))
        n, r = h, r + 1
    return out, a[0], b[0]


# ------------------------------------------------------------------ events
class Events(dict):
    """(site, event) -> count; `where` lists (site, event, tag) of the additions that carry a tag"""

    def __init__(self):
        super().__init__()
        self.where = []

    def hit(self, site, ev, tag=None):
        self[(site, ev)] = self.get((site, ev), 0) + 1
        if tag is not None:
            self.where.append((site, ev, tag))

    def add(self, site, acc, q, held=True, tag=None):
        """acc + q on logarithms; held False: an accumulator that has not yet held a point does not count as an identity operand"""
        if q == 0 or (acc == 0 and held):
            self.hit(site, "ident", tag)
        elif acc == q:
            self.hit(site, "dbl", tag)
        elif (acc + q) % N == 0 and acc:
            self.hit(site, "cancel", tag)
        return (acc + q) % N

    def merge(self, other):
        for k, v in other.items():
            self[k] = self.get(k, 0) + v
        self.where += other.where
        return self

    def count(self, site, ev):
        return self.get((site, ev), 0)

    def identity_partials(self, site):
        """the `ident` of the strided pass over chunk partial sums: an identity partial, or one that meets a lane's lost sum"""
        return sum(1 for s, e, tag in self.where if s == site and e == "ident" and tag[0] == "stride")


# ------------------------------------------------------------------ the round MSMs over resident generators
def ipp_launch(c, n0, nmsm):
    """fixed_msm_ipp_chunks and launch_fixed_ipp (csrc/k_fixed.hip)"""
    W = wd.windows(c)
    total = (1 + n0) * W
    grouped = nmsm >= 16
    if grouped:
        units = 2 * ((nmsm // 2 + 7) // 8)
        chunks = min((total + 255) // 256, (2048 + units - 1) // units)
    else:
        chunks = min((total + 511) // 512, (1024 + nmsm - 1) // nmsm)
    chunks = max(chunks, 1)
    per = -(-total // chunks)
    if grouped:
        per = (per + 7) & ~7
    return dict(c=c, n0=n0, W=W, total=total, grouped=grouped, chunks=chunks, per=per, stride=8 if grouped else 128)


# (c, n0, nb) -> (grouped, chunks, pairs per chunk), and the cases that are placed by these numbers
LAUNCHES = {
    (8, 16, 3): (False, 2, 272, "B.2 block-kernel placements (pair_msms) and the 2-partial tail"),
    (8, 16, 8): (True, 3, 184, "B.2 grouped-kernel placements (pair_msms) and the 3-partial tail"),
    (8, 16, 9): (True, 3, 184, "B.1 nb = 9: the second unit with one live lane"),
    (8, 128, 8): (True, 17, 248, "B.4 seventeen_chunk_case: the pairs at chunks (0, 16) and (3, 11)"),
    (16, 16, 3): (False, 1, 272, "B.2 at c = 16, block kernel"),
    (16, 16, 8): (True, 2, 136, "B.2 at c = 16, grouped kernel"),
}


def chunk_of(launch, t, w):
    return (t * launch["W"] + w) // launch["per"]


def shadow_msm(terms, launch, ev):
    """terms: [(scalar, logarithm of its generator)] in compact order -> the chunk partial sums"""
    W, c, per, stride = launch["W"], launch["c"], launch["per"], launch["stride"]
    assert len(terms) * W == launch["total"]
    digs = [wd.digits(s % N, c) if s % N else None for s, _ in terms]
    partials = []
    for ch in range(launch["chunks"]):
        lo, hi = ch * per, min(ch * per + per, launch["total"])
        acc, held = [0] * stride, [False] * stride
        for ll in range(lo, hi):
            t, w = divmod(ll, W)
            d = digs[t][w] if digs[t] else 0
            if d:
                q = d * (1 << (c * w)) * terms[t][1] % N
                assert q          # (the tables of these cases hold no identity generator)
                lane = (ll - lo) % stride
                acc[lane] = ev.add("lane", acc[lane], q, held[lane])
                held[lane] = True
        if launch["grouped"]:      # offsets 8, 16, 32 of the wave: bits 0, 1, 2 of the pair-lane; the adds that reach pair-lane 0
            for s in (1, 2, 4):
                for pl in range(0, 8, 2 * s):
                    acc[pl] = ev.add("reduce", acc[pl], acc[pl + s])
        else:
            _block_sum(acc, ev, "reduce")
        partials.append(acc[0])
    return partials


def _block_sum(acc, ev, site, tag=None):
    s = len(acc) // 2
    while s:
        for tid in range(s):
            acc[tid] = ev.add(site, acc[tid], acc[tid + s], tag=None if tag is None else (tag, s, tid))
        s //= 2


def shadow_segmented_sum(partials, ev):
    """k_segmented_sum<16> (chunk counts up to 64)"""
    assert 1 < len(partials) <= 64
    acc = [0] * 16
    for i, q in enumerate(partials):          # (a lane's first addition meets an empty accumulator: `ident` there is an identity PARTIAL)
        acc[i % 16] = ev.add("partials", acc[i % 16], q, held=i >= 16, tag=("stride", i % 16, i // 16))
    _block_sum(acc, ev, "partials")
    if acc[0] == 0:
        ev.hit("partials", "zero_out")
    return acc[0]


def shadow_tail(partials, ev):
    """k_ipp_round_tail, one side: tags ("stride", lane, iteration) and ("bfly", offset, lane)"""
    assert 1 < len(partials) <= 256
    acc = [0] * 16
    for i, q in enumerate(partials):          # (as in shadow_segmented_sum: the first addition of a lane does not count its empty accumulator)
        acc[i % 16] = ev.add("tail", acc[i % 16], q, held=i >= 16, tag=("stride", i % 16, i // 16))
    _block_sum(acc, ev, "tail", tag="bfly")
    if acc[0] == 0:
        ev.hit("tail", "zero_out")
    return acc[0]


class Resident:
    """a resident-generator session on logarithms: the coefficient bookkeeping of k_ipp_gens_scalars / k_ipp_gens_fold"""

    def __init__(self, case):
        self.case, self.n0, self.cur = case, case.n, case.n
        self.a = [list(v) for v in case.a]
        self.b = [list(v) for v in case.b]
        self.cG = [list(v) for v in case.gf]
        self.cH = [list(v) for v in case.hf]

    def terms(self, p):
        """-> (L terms, R terms), compact order: the scalar goes where k_ipp_gens_scalars stores it, the generator is the one
        k_fixed_msm_ipp's enumeration reads for that term"""
        cs, n0, cur = self.case, self.n0, self.cur
        h, half = cur // 2, n0 // 2
        a, b = self.a[p], self.b[p]
        Ls, Rs = [0] * (1 + n0), [0] * (1 + n0)
        for i in range(n0):
            t = i % cur
            tl, hi = t % h, t % cur >= h
            j = (i // cur) * h + tl
            if hi:
                Ls[1 + j] = a[tl] * self.cG[p][i] % N
                Rs[1 + half + j] = b[tl] * self.cH[p][i] % N
            else:
                Ls[1 + half + j] = b[h + tl] * self.cH[p][i] % N
                Rs[1 + j] = a[h + tl] * self.cG[p][i] % N
        Ls[0] = dot(a[:h], b[h:cur]) * cs.w[p] % N
        Rs[0] = dot(a[h:cur], b[:h]) * cs.w[p] % N

        def gen(t, is_R):
            if t == 0:
                return cs.kB
            isH = t - 1 >= half
            j = t - 1 - half if isH else t - 1
            use_hi = isH if is_R else not isH
            i = (j // h) * cur + (h if use_hi else 0) + j % h
            return (cs.kH if isH else cs.kG)[i]
        return ([(s, gen(t, False)) for t, s in enumerate(Ls)], [(s, gen(t, True)) for t, s in enumerate(Rs)])

    def fold(self, us):
        cur, h = self.cur, self.cur // 2
        for p in range(self.case.nb):
            u, ui = us[p], inv(us[p])
            for i in range(self.n0):
                hi = i % cur >= h
                self.cG[p][i] = self.cG[p][i] * (u if hi else ui) % N
                self.cH[p][i] = self.cH[p][i] * (ui if hi else u) % N
            a, b = self.a[p], self.b[p]
            self.a[p] = [(a[i] * u + a[h + i] * ui) % N for i in range(h)]
            self.b[p] = [(b[i] * ui + b[h + i] * u) % N for i in range(h)]
        self.cur = h

    def folded_gens(self, p):
        return dot(self.cG[p], self.case.kG), dot(self.cH[p], self.case.kH)


def shadow_resident_round(res, launch, tail):
    """the current round of every proof -> (events, [(L, R)] as logarithms)"""
    ev, out = Events(), []
    for p in range(res.case.nb):
        lr = []
        for terms in res.terms(p):
            part = shadow_msm(terms, launch, ev)
            want = sum(s * k for s, k in terms) % N
            if launch["chunks"] == 1:
                got = part[0]
                if got == 0:
                    ev.hit("partials", "zero_out")
            else:
                got = shadow_tail(part, ev) if tail else shadow_segmented_sum(part, ev)
            assert got == want
            lr.append(got)
        out.append(tuple(lr))
    return ev, out


# ------------------------------------------------------------------ A: sessions over explicit generators
def _rand(rnd, k):
    return [rnd.randrange(1, N) for _ in range(k)]


def random_case(name, n, nb, seed, shared=False, one_u=False):
    rnd = random.Random(seed)
    kG = _rand(rnd, n) if shared else [_rand(rnd, n) for _ in range(nb)]
    kH = _rand(rnd, n) if shared else [_rand(rnd, n) for _ in range(nb)]
    k = n.bit_length() - 1
    us = [_rand(rnd, nb) for _ in range(k)]
    if one_u:
        us = [[r[0]] * nb for r in us]
    def rows():
        return [_rand(rnd, n) for _ in range(nb)]
    return Case(name=name, n=n, nb=nb, kG=kG, kH=kH, q=_rand(rnd, nb), gf=rows(), hf=rows(), a=rows(), b=rows(), us=us, shared=shared)


# A.1: flat indices p h + i (of the fold that produces them) of the folded generators that are the identity
FOLD_IDENTITIES = {
    # n = 16, nb = 3: h = 8, 24 lanes, three full runs
    ("first", 16): dict(G=[0, 3, 7] + list(range(8, 16)), H=[9] + list(range(16, 24))),
    # n = 8, nb = 3: h = 4, 12 lanes: a run of 8 and the short run 8..11
    ("first", 8): dict(G=[2, 8, 11], H=[0, 7, 8, 9, 10, 11]),
    # n = 16, nb = 3, the SECOND fold: h = 4, 12 lanes again, scalars broadcast
    ("later", 16): dict(G=[0, 4, 7, 10], H=[3, 8, 9, 10, 11]),
}


def fold_identity_case(which, n, shared, seed=None):
    """A.1.  first: k_{h+i} := -u^-2 gf_i k_i / gf_{h+i} (H: -u^2 hf_i k_i / hf_{h+i}) at the listed positions, so that the first
    fold gives the identity there.  later: the same for the second fold, solved for the first round's k_{h+j}.  With shared
    generators the proofs share k, so the FACTOR gf_{p, h+i} is solved for instead, under one u for all proofs."""
    nb = 3
    cs = random_case("fold_identities_%s_n%d_%s" % (which, n, "shared" if shared else "own"), n, nb,
                     seed if seed is not None else 5100 + n + (7 if shared else 0) + (13 if which == "later" else 0), shared, one_u=shared)
    cs.which, cs.placed = which, FOLD_IDENTITIES[(which, n)]
    h = n // 2
    for side in "GH":
        for f in cs.placed[side]:
            fac = cs.gf if side == "G" else cs.hf
            if which == "first":
                p, i = divmod(f, h)
                j, target = i, 0
            else:
                p, i = divmod(f, h // 2)
                j = h // 2 + i
            k = cs.gens_of(p)[0 if side == "G" else 1]
            u0 = cs.us[0][p]
            lft, rgt = (inv(u0), u0) if side == "G" else (u0, inv(u0))       # G' = u^-1 G_L + u G_R, H' = u H_L + u^-1 H_R
            if which == "later":
                u1 = cs.us[1][p]
                l1, r1 = (inv(u1), u1) if side == "G" else (u1, inv(u1))
                first_i = (lft * fac[p][i] * k[i] + rgt * fac[p][h + i] * k[h + i]) % N
                target = -l1 * inv(r1) * first_i % N
            rest = (target - lft * fac[p][j] * k[j]) * inv(rgt) % N      # = fac_{h+j} k_{h+j}
            if shared:
                fac[p][h + j] = rest * inv(k[h + j]) % N
            else:
                k[h + j] = rest * inv(fac[p][h + j]) % N
            assert fac[p][h + j] and k[h + j]
    return cs


def run_positions(flat, total):
    """the identity positions `flat` among `total` points in runs of 8 -> the set of placements they make"""
    out, s = set(), set(flat)
    nruns = -(-total // 8)
    whole = [all(8 * r + i in s for i in range(min(8, total - 8 * r))) for r in range(nruns)]
    some = [any(8 * r + i in s for i in range(8)) for r in range(nruns)]
    for r in range(nruns):
        ln = min(8, total - 8 * r)
        if ln < 8 and some[r]:
            out.add("short")
        if whole[r]:
            out.add("whole")
            if any(0 <= r2 < nruns and not whole[r2] for r2 in (r - 1, r + 1)):
                out.add("whole_next_to_partial")
            continue
        for i in range(ln):
            if 8 * r + i in s:
                out.add("first" if i == 0 else "last" if i == ln - 1 else "middle")
    return out


def fold_lane_scalars(cs, r, p, i, side, h):
    """the two scalars of fold lane (p, i) of round r as ipp_fold_dev passes them to straus<2>"""
    u = cs.us[r][p]
    lft, rgt = (inv(u), u) if side == "G" else (u, inv(u))
    if r == 0:
        fac = cs.gf[p] if side == "G" else cs.hf[p]
        return lft * fac[i] % N, rgt * fac[h + i] % N
    return lft, rgt


def shadow_fold(cs, r, side, gens_before):
    """straus_body<2> over the nb h lanes of round r's fold.  gens_before[p]: the generators' logarithms going in (without factors).
    -> (events, flat list of the folded logarithms, [wave -> skip bits])"""
    ev = Events()
    h = len(gens_before[0]) // 2
    lanes = [(p, i) for p in range(cs.nb) for i in range(h)]
    out, skips = [], []
    for w0 in range(0, len(lanes), 64):
        wave = lanes[w0:w0 + 64]
        wave += [wave[-1]] * (64 - len(wave))          # (dead lanes are clamped to the last live one)
        skip = [all(gens_before[p][j * h + i] == 0 for p, i in wave) for j in (0, 1)]
        skips.append(tuple(skip))
        for p, i in lanes[w0:w0 + 64]:
            k = (gens_before[p][i], gens_before[p][h + i])
            sc = fold_lane_scalars(cs, r, p, i, side, h)
            dg = [wd.digits(s, 4) for s in sc]
            for j in (0, 1):
                if k[j] == 0:
                    ev.hit("fold_lane", "ident")           # pinf (or skip)
            acc, held = 0, False
            for w in range(63, -1, -1):
                if w != 63:
                    acc = acc * 16 % N
                for j in (0, 1):
                    if dg[j][w] and k[j]:
                        acc = ev.add("fold_lane", acc, dg[j][w] * k[j] % N, held)
                        held = True
            assert acc == (sc[0] * k[0] + sc[1] * k[1]) % N
            if acc == 0:
                ev.hit("fold_lane", "zero_out")
            out.append(acc)
    return ev, out, skips


def gens_before_round(cs, r):
    """per proof, (G, H) logarithms as the session holds them before round r's fold: the input generators for r = 0 (factors apart),
    the folded ones after"""
    if r == 0:
        return [list(cs.gens_of(p)[0]) for p in range(cs.nb)], [list(cs.gens_of(p)[1]) for p in range(cs.nb)]
    G, H = [], []
    for p in range(cs.nb):
        rr = rounds(cs, p)[0][r - 1]
        G.append(rr[2])
        H.append(rr[3])
    return G, H


def multiples_case():
    """A.2: lanes whose right generator is the left one, its negative or its double, in turn with an unrelated one.  Proof 0: factors
    1 and u = 1 in every round (both scalars are 1: the same digits in every window); proof 1: u = 1 and equal factors on both
    halves; proof 2: random factors and challenges."""
    n, nb = 8, 3
    cs = random_case("multiples_inside_a_fold_lane", n, nb, 5200)
    h = n // 2
    mult = (1, -1, 2, None)
    for p in range(nb):
        for side in (cs.kG[p], cs.kH[p]):
            for i in range(h):
                m = mult[(i + p) % 4]
                if m is not None:
                    side[h + i] = m * side[i] % N
    cs.gf[0], cs.hf[0] = [1] * n, [1] * n
    cs.gf[1] = cs.gf[1][:h] * 2
    cs.hf[1] = cs.hf[1][:h] * 2
    for r in range(len(cs.us)):
        cs.us[r][0] = cs.us[r][1] = 1
    return cs


def identity_inputs_case():
    """A.3: nb = 8, n = 32, own generators: h = 16, so the first fold has 128 lanes, two waves.  G: the left point of every lane of
    wave 0 (proofs 0..3) is the identity -- `skip` -- and wave 1 has identity left or right points in some lanes -- `pinf`.  H: the
    other way round, with the RIGHT points of wave 1.  A zero G factor and a zero H factor sit on ordinary generators."""
    n, nb = 32, 8
    cs = random_case("identity_input_generators", n, nb, 5300)
    h = n // 2
    for p in range(4):
        for i in range(h):
            cs.kG[p][i] = 0
            cs.kH[p + 4][h + i] = 0
    for p, i in ((4, 0), (4, h + 3), (5, 7), (5, h + 7), (6, h), (7, 15), (7, h + 15)):
        cs.kG[p][i] = 0
        cs.kH[p - 4][(i + h + 1) % n] = 0
    cs.gf[5][2] = cs.gf[1][h + 4] = 0
    cs.hf[6][h + 1] = cs.hf[2][5] = 0
    return cs


def zero_halves_case(n=8, shared=False):
    """A.4, nb = 3: proof 0 has a_L = 0 and b_R = 0 (L = the identity, c_L = 0, R ordinary), proof 1 is all zero (L = R = the identity
    in every round), proof 2 has a_R = 0 and b_L = 0 (R = the identity).  Q is an ordinary point, so a wrong c_L or c_R shows.
    shared: one generator set, as a resident-generator session needs it (c = 8, Q = w B)."""
    cs = random_case("zero_halves", n, 3, 5400 + n, shared=shared)
    h = n // 2
    cs.a[0][:h], cs.b[0][h:] = [0] * h, [0] * h
    cs.a[1], cs.b[1] = [0] * n, [0] * n
    cs.a[2][h:], cs.b[2][:h] = [0] * h, [0] * h
    if shared:
        cs.c, cs.kB, cs.w = 8, 1, list(cs.q)
    return cs


# ------------------------------------------------------------------ B: resident-generator sessions
KB = 0x5DEECE66D1234567890ABCDEF0FEDCBA9876543210F00DFACE          # B_blinding (unused by the rounds)
KP, KQ = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA998877, 0x7A6B5C4D3E2F10213243546576879809A0B1C2D3E4F5


def coinciding_table(c):
    """capacity 16: the logarithms of G and H so that the compact terms 1..16 of a first-round L (G_8.., H_0..) and R (G_0.., H_8..)
    read the same pattern KT: P in many places, Q and -Q, and 2^c P (whose digit d in window w is P's digit d in window w + 1)"""
    p, q, sh = KP, KQ, (KP << c) % N
    KT = [None, p, p, p, sh, p, q, N - q, p, p, N - q, q, p, p, p, N - p, q]
    kG = KT[1:9] + KT[1:9]
    kH = KT[9:17] + KT[9:17]
    return KT, kG, kH


def one(c, w, d):
    """the scalar whose only digits are d in window w (and the carry 1 in window w + 1 for d < 0)"""
    return ((d << (c * w)) + ((1 << (c * (w + 1))) if d < 0 else 0)) % N


def _digit_set(c):
    return (1, (1 << (c - 1)) - 1, -(1 << (c - 1)))


def pair_candidates(c):
    """MSMs {term: scalar} over coinciding_table(c): two (three) terms whose rows coincide or are opposite in one window, and
    whole MSMs that cancel"""
    W = wd.windows(c)
    KT = coinciding_table(c)[0]
    ws = sorted({0, 1, 7, W // 2 - 1, W // 2, W - 3})
    out = []
    for t1 in range(1, 17):
        for t2 in range(t1 + 1, 17):
            k1, k2 = KT[t1], KT[t2]
            for w, d in ((w, d) for w in ws for d in _digit_set(c)):
                if k1 == k2:
                    out.append({t1: one(c, w, d), t2: one(c, w, d)})
                    if d != -(1 << (c - 1)):
                        out.append({t1: one(c, w, d), t2: one(c, w, -d)})
                        for t3 in range(t2 + 1, 17):                      # an accumulator that cancelled meets a third row
                            out.append({t1: one(c, w, d), t2: one(c, w, -d), t3: one(c, w, 1)})
                elif (k1 + k2) % N == 0:
                    out.append({t1: one(c, w, d), t2: one(c, w, d)})
                elif k2 == (k1 << c) % N:
                    out.append({t1: one(c, w + 1, d), t2: one(c, w, d)})
                    if d != -(1 << (c - 1)):
                        out.append({t1: one(c, w + 1, d), t2: one(c, w, -d)})
                elif k1 == (k2 << c) % N:
                    out.append({t1: one(c, w, d), t2: one(c, w + 1, d)})
            top = wd.top_digit(c)
            if k1 == k2:
                out.append({t1: top << (c * (W - 1)), t2: top << (c * (W - 1))})
    rnd = random.Random(5500 + c)
    bat = list(wd.battery(c).values())
    for s in bat[::11] + [rnd.randrange(1, N)]:          # whole MSMs that cancel
        out += [{1: s, 2: N - s}, {1: s, 13: N - s}, {6: s, 7: s}, {3: s, 15: s}, {6: s, 10: s}]
    rnd.shuffle(out)            # (so that the first hits of pair_msms vary in terms, windows and digits)
    return out


def msm_of(c, case_msm, w_scalar=0):
    """{term: scalar} -> the 17 compact terms over coinciding_table(c) with B's scalar"""
    KT = coinciding_table(c)[0]
    return [(w_scalar, 1)] + [(case_msm.get(t, 0), KT[t]) for t in range(1, 17)]


WANTED = [(site, e) for site in ("lane", "reduce", "partials") for e in ("dbl", "cancel", "ident")] + [("partials", "zero_out")]


@functools.lru_cache(maxsize=None)
def pair_msms(c, nb, per_kind=3):
    """B.2: from pair_candidates(c), per (site, event) of WANTED the first `per_kind` MSMs whose shadow under the launch of nb
    provers has that event -- an `ident` in a lane accumulator, a `dbl` or `cancel` anywhere: the identity operands of sparse
    sums come by themselves -- in candidate order, digits and windows in turn.  -> [{term: scalar}]"""
    launch = ipp_launch(c, 16, 2 * nb)
    picked, have = [], {k: 0 for k in WANTED}
    for m in pair_candidates(c):
        ev = Events()
        part = shadow_msm(msm_of(c, m), launch, ev)
        if launch["chunks"] > 1:
            shadow_segmented_sum(part, ev)
        elif part[0] == 0:
            ev.hit("partials", "zero_out")
        new = [k for k in WANTED if ev.count(*k) and have[k] < per_kind
               and (k[1] in ("dbl", "cancel", "zero_out") or k == ("lane", "ident"))]
        if new:
            picked.append(m)
            for k in WANTED:
                if ev.count(*k):
                    have[k] += 1
    top = wd.top_digit(c) << (c * (wd.windows(c) - 1))
    return picked + [{1: top, 2: top}, {6: top, 7: top}, {2: top, 14: top}]         # P + P and Q - Q on the top-window rows


def provers_of(c, msms, nb, seed, fill=None):
    """lay MSMs out as provers' first rounds, factors 1: prover p's L is msms[2p], its R msms[2p + 1] (a = a_L | a_R, b = b_L | b_R;
    L walks a_L on the G terms 1..8 and b_R on the H terms 9..16, R walks a_R and b_L).  Sessions of nb provers; a last short
    session is filled up with `fill` MSMs (default: repeat from the start).  -> [Case]"""
    KT, kG, kH = coinciding_table(c)
    rnd = random.Random(seed)
    msms = list(msms)
    while len(msms) % (2 * nb):
        msms.append((fill or msms)[len(msms) % len(fill or msms)])
    out = []
    for s0 in range(0, len(msms), 2 * nb):
        a, b = [], []
        for p in range(nb):
            L, R = msms[s0 + 2 * p], msms[s0 + 2 * p + 1]
            a.append([L.get(1 + j, 0) for j in range(8)] + [R.get(1 + j, 0) for j in range(8)])
            b.append([R.get(9 + j, 0) for j in range(8)] + [L.get(9 + j, 0) for j in range(8)])
        k = 4
        w = _rand(rnd, nb)
        ones = [[1] * 16 for _ in range(nb)]
        out.append(Case(name="coinciding_c%d_nb%d_%d" % (c, nb, s0 // (2 * nb)), n=16, nb=nb, kG=kG, kH=kH, q=list(w), gf=ones,
                        hf=[list(r) for r in ones], a=a, b=b, us=[_rand(rnd, nb) for _ in range(k)], shared=True, c=c, kB=1, w=w))
    return out


def coinciding_cases(c, nb):
    return provers_of(c, pair_msms(c, 3 if nb < 8 else 8), nb, 5600 + 16 * c + nb)


def zero_proof_case(c, nb):
    """an all-zero proof (prover 1) between ordinary ones over coinciding_table(c)"""
    cs = random_case("zero_proof_c%d_nb%d" % (c, nb), 16, nb, 5700 + c + nb, shared=True)
    cs.kG, cs.kH = coinciding_table(c)[1:]
    cs.a[1], cs.b[1] = [0] * 16, [0] * 16
    cs.c, cs.kB, cs.w = c, 1, list(cs.q)
    return cs


def battery_rounds_case(c, nb, u_one, seed=5800):
    """B.3: n0 = 16 over distinct generators with factors 1.  The vectors of round 2 (length 8) hold battery(c) scalars, n - 1 and
    zeros, placed so that round 3's vectors (a_L u + a_R u^-1 with u = 1: one of the two is zero) are battery scalars too; round 1's
    are a battery scalar and the difference that folds to round 2's.  u_one: every challenge is 1, the coefficients stay 1 and the
    MSM scalars of round r ARE the folded vectors; else the test's own challenges, the coefficients become products of u, u^-1."""
    rnd = random.Random(seed + c + nb)
    bat = [N - 1] + list(wd.battery(c).values())
    it = [-1]

    def nxt():
        it[0] += 1
        return bat[(37 * it[0]) % len(bat)]           # (the first draw, N - 1, goes into round 2's and 3's vector)
    a, b = [], []
    for p in range(nb):
        vecs = []
        for _ in range(2):
            v2 = [0] * 8
            for i in range(4):
                v2[i + 4 * ((i + p) % 2)] = nxt()             # one of v2[i], v2[4 + i] is zero: round 3's entry is the other
            r = [nxt() for _ in range(8)]
            vecs.append(r + [(v2[i] - r[i]) % N for i in range(8)])
        a.append(vecs[0])
        b.append(vecs[1])
    gr = random.Random(seed + c)                     # (one generator table per c for all of these sessions)
    kG, kH = _rand(gr, 16), _rand(gr, 16)
    us = [[1] * nb for _ in range(4)] if u_one else [_rand(rnd, nb) for _ in range(4)]
    w = _rand(rnd, nb)
    return Case(name="battery_rounds_c%d_nb%d_%s" % (c, nb, "u1" if u_one else "u"), n=16, nb=nb, kG=kG, kH=kH, q=list(w),
                gf=[[1] * 16 for _ in range(nb)], hf=[[1] * 16 for _ in range(nb)], a=a, b=b, us=us, shared=True, c=c, kB=1, w=w)


def seventeen_chunk_case():
    """B.4: n0 = cap = 128, c = 8, nb = 8: 4 128 pairs in 17 chunks of 248.  Terms 1 and 125 lie wholly in chunks 0 and 16, terms 24
    and 86 in chunks 3 and 11; their generators are all P.  Prover 0: L has the same one-digit scalar on 1 and 125 (lane 0 of the
    tail adds two equal partial sums in its strided pass) and R the same on 24 and 86 (equal partials meet in the butterfly at
    offset 8).  Prover 1: opposite scalars in the same places, L and R are the identity.  Prover 2: both pairs in L, opposite
    ones in R.  Prover 3: all zero.  Provers 4..7: ordinary."""
    n, nb, c = 128, 8, 8
    cs = random_case("seventeen_chunks", n, nb, 5900, shared=True)
    half = n // 2
    T = {1: None, 125: None, 24: None, 86: None}
    for t in T:            # compact term -> (vector, index) of L and of R in the first round
        T[t] = ("G", t - 1) if t <= half else ("H", t - 1 - half)
    for t, (side, j) in T.items():       # L reads G_hi[j] = G_{64+j} and H_lo[j]; R reads G_lo[j] and H_hi[j] = H_{64+j}
        if side == "G":
            cs.kG[j] = cs.kG[half + j] = KP
        else:
            cs.kH[j] = cs.kH[half + j] = KP
    s1, s2 = one(c, 5, 127), one(c, 30, -128)

    def put(p, is_R, t, s):
        side, j = T[t]
        if side == "G":
            cs.a[p][(half if is_R else 0) + j] = s       # L: a_L on G_hi; R: a_R on G_lo
        else:
            cs.b[p][(0 if is_R else half) + j] = s       # L: b_R on H_lo; R: b_L on H_hi
    for p in range(4):
        cs.a[p], cs.b[p] = [0] * n, [0] * n
    put(0, False, 1, s1), put(0, False, 125, s1), put(0, True, 24, s2), put(0, True, 86, s2)
    put(1, False, 1, s1), put(1, False, 125, N - s1), put(1, True, 24, s2), put(1, True, 86, N - s2)
    put(2, False, 1, s1), put(2, False, 125, s1), put(2, False, 24, s2), put(2, False, 86, s2)
    put(2, True, 1, s2), put(2, True, 125, N - s2), put(2, True, 24, s1), put(2, True, 86, N - s1)
    cs.gf, cs.hf = [[1] * n for _ in range(nb)], [[1] * n for _ in range(nb)]
    cs.c, cs.kB, cs.w = c, 1, list(cs.q)
    return cs


def folded_gens_cases(c):
    """B.5: sessions over coinciding_table(c) whose G coefficients cancel on the coinciding G_0 = G_8 = P (G' = the identity) or are
    equal there (G' = 2 cG_0 P), every other G factor zero; H likewise on H_0 = H_8.  The factors are solved from the test's
    challenges: after the four folds cG_0 = gf_0 / (u_1 u_2 u_3 u_4) and cG_8 = gf_8 u_1 / (u_2 u_3 u_4)."""
    out = []
    for kind in ("cancel", "double"):
        nb = 3
        cs = random_case("folded_gens_%s_c%d" % (kind, c), 16, nb, 6000 + c, shared=True)
        cs.kG, cs.kH = coinciding_table(c)[1:]
        for p in range(nb):
            u1 = cs.us[0][p]
            sign = N - 1 if (kind == "cancel" and p != 2) else 1         # (proof 2 of `cancel` doubles G and cancels H)
            g0, h0 = cs.gf[p][0], cs.hf[p][0]
            cs.gf[p], cs.hf[p] = [0] * 16, [0] * 16
            cs.gf[p][0], cs.gf[p][8] = g0, sign * g0 * inv(u1) * inv(u1) % N
            hs = N - 1 if (kind == "cancel" and p == 2) else 1
            cs.hf[p][0], cs.hf[p][8] = h0, hs * h0 * u1 * u1 % N
        cs.c, cs.kB, cs.w = c, 1, list(cs.q)
        out.append(cs)
    return out


# ------------------------------------------------------------------ what the committed cases reach
def coverage():
    """-> {name: Events} of the committed B cases and the A fold cases (the numbers of the module docstring)"""
    out = {}
    for nb, key in ((3, "block"), (8, "grouped")):
        tot = Events()
        for cs in coinciding_cases(8, nb):
            ev, _ = shadow_resident_round(Resident(cs), ipp_launch(8, 16, 2 * nb), tail=False)
            tot.merge(ev)
        out[key] = tot
    for nb in (3, 8):
        tot = Events()
        for cs in coinciding_cases(8, nb) + [zero_proof_case(8, nb)]:
            ev, _ = shadow_resident_round(Resident(cs), ipp_launch(8, 16, 2 * nb), tail=True)
            tot.merge(ev)
        out["tail%d" % ipp_launch(8, 16, 2 * nb)["chunks"]] = tot
    cs = seventeen_chunk_case()
    out["tail17"] = shadow_resident_round(Resident(cs), ipp_launch(8, 128, 16), tail=True)[0]
    tot = Events()
    for cs in (multiples_case(), identity_inputs_case()):
        G, H = gens_before_round(cs, 0)
        tot.merge(shadow_fold(cs, 0, "G", G)[0]).merge(shadow_fold(cs, 0, "H", H)[0])
    out["fold"] = tot
    return out


if __name__ == "__main__":
    for name, ev in coverage().items():
        print(name, {k: v for k, v in sorted(ev.items())}, "identity partials:", ev.identity_partials("tail" if "tail" in name else "partials"))
