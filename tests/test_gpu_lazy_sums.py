"""The lazy F_n sums of the scalar kernels on the device, at their budgets and across their fold boundaries (tests/lazy_sum_cases.py:
the operands, the lengths and why; tests/test_lazy_sums_cpu.py: the same shapes on a CPU build, and the measured headroom).  Every
product is the heaviest one -- lazily n - 1 -- on the indices a family selects, the lengths put the loops' fn_reduce on the last trip,
in mid-loop, and on some lanes only, and every result is compared byte for byte with Python integers or the CPU oracle:
bpgpu_inner_product (second grid stride, in-loop fold), c_L / c_R of an IPP round (k_sc_dot_batched), the prover's t-coefficients
(k_prover_tcoeffs, raw planes), and one party's Beaver combines of the two-party prover (k_mpc_tcoeffs, k_mpc_ipp_combine).
Run with `-m gpu` on an MI355X."""
import functools
import random

import pytest

import circuit_gen as cg
import lazy_sum_cases as lz
import mpc_dealer as md
import oracle_lib as o
from polys_model import model_polys, padded

pytestmark = pytest.mark.gpu
N, C = lz.N, lz.C
le, unmont, cut = md.le, md.unmont, md.cut
mont = functools.lru_cache(maxsize=1 << 16)(md.mont)
MPC_CAP = 8192


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def points():
    """2 x 16 384 + 1 distinct points, cheaply: a chain of additions over eight of the oracle's generators"""
    step = cut(o.gens("G", 9), 64)
    out, p = [], step[8]
    for i in range(2 * 16384 + 1):
        out.append(p)
        p = o.point_add(p, step[i % 8])
    assert len(set(out)) == len(out)
    return out


@pytest.fixture(scope="module")
def mpc_gens(gpu, points):
    """resident generators over the cheap points, 4-bit windows (the table of 2 x 8192 generators stays small)"""
    g = gpu.gens_create(b"".join(points[:MPC_CAP]), b"".join(points[16384:16384 + MPC_CAP]), o.generator(), o.generator(), 4)
    yield g
    gpu.gens_destroy(g)


def ints(b):
    return [int.from_bytes(x, "little") for x in cut(b, 32)]


def pack(vals):
    return b"".join(le(v) for v in vals)


# ------------------------------------------------------------------------------------------------ bpgpu_inner_product
@pytest.mark.parametrize("n", lz.ip_lengths())
def test_inner_product_second_stride_and_in_loop_fold(gpu, n):
    stride = lz.IP_MAX_BLOCKS * lz.TPB
    assert n in (stride - 1, stride + 1, 2 * stride + 77, 16 * stride, 16 * stride + 1000)
    rnd = random.Random(n)
    for fam in lz.families(n, rnd, stride):
        got = gpu.inner_product(fam.a_bytes(), fam.b_bytes())
        assert got == le(fam.want()), ("inner_product", fam.name, fam.at, n)
    if n < 2 * stride:
        a, b = o.random_scalars(n, n), o.random_scalars(n + 1, n)
        assert gpu.inner_product(a, b) == o.inner_product(a, b), ("inner_product", "random", n)


# ------------------------------------------------------------------------------------------------ k_sc_dot_batched: c_L, c_R
@pytest.mark.parametrize("n", lz.dot_ipp_lengths())
def test_ipp_round_dot_products_at_the_fold(gpu, points, n):
    """one bpgpu_ipp_round of two proofs over n generators (the literal schedule: no tables to build): proof 0 pairs a_L with b_R and
    a_R with b_L so that every product is the heaviest, proof 1 is proof 0 with b zeroed on the odd indices.  L, R of proof 0 are the
    oracle's MSMs over the round's 2h + 1 terms; proof 1's follow from them by linearity (minus the odd H terms, and the change of c)."""
    assert n in (8192, 16384)
    h, nb = n // 2, 2
    rnd = random.Random(n)
    G, H, Q = points[:n], points[16384:16384 + n], points[2 * 16384]
    famL, famR = lz.Family("worst", h, rnd), lz.Family("worst", h, rnd)
    aL, bR, aR, bL = famL.a_list(), famL.b_list(), famR.a_list(), famR.b_list()
    even = lambda v: [x if i % 2 == 0 else 0 for i, x in enumerate(v)]      # noqa: E731
    a = pack(aL + aR) * 2
    b = pack(bL + bR) + pack(even(bL) + even(bR))
    ones = pack([1]) * (nb * n)
    old = gpu.get_option("ipp_literal")
    gpu.set_option("ipp_literal", 1)
    try:
        s = gpu.ipp_begin(nb, n, Q * nb, ones, ones, b"".join(G), b"".join(H), True, a, b)
        try:
            L, R = gpu.ipp_round(s, nb)
        finally:
            gpu.ipp_destroy(s)
    finally:
        gpu.set_option("ipp_literal", old)
    cL, cR = famL.want(), famR.want()
    assert cL == cR == h * C % N
    wantL = o.msm(pack(aL + bR + [cL]), b"".join(G[h:] + H[:h] + [Q]))
    wantR = o.msm(pack(aR + bL + [cR]), b"".join(G[:h] + H[h:] + [Q]))
    assert (L[:64], R[:64]) == (wantL, wantR), ("sc_dot_batched", "worst", n)
    # worst_even: the odd b terms leave the MSM and c drops to the even indices' share
    cE = (h + 1) // 2 * C % N
    odd = list(range(1, h, 2))
    dL = o.msm(pack([-bR[i] for i in odd] + [cE - cL]), b"".join([H[i] for i in odd] + [Q]))
    dR = o.msm(pack([-bL[i] for i in odd] + [cE - cR]), b"".join([H[h + i] for i in odd] + [Q]))
    assert (L[64:], R[64:]) == (o.point_add(wantL, dL), o.point_add(wantR, dR)), ("sc_dot_batched", "worst_even", n)


# ------------------------------------------------------------------------------------------------ k_prover_tcoeffs
def sparse_circuit(n):
    """three short rows over n multipliers: the flattened weights vanish at all but a few indices, so the planes are the witness"""
    return cg.Circuit(700 + n, n, 0, 1, 3, 0, "sparse")


def witnesses(n, rnd, stride):
    """(family name, position, witness per y) for y = 1 and y = n - 1"""
    out = []
    for fam in lz.families(n, rnd, stride):
        out.append((fam.name, fam.at, [lz.tcoeffs_witness(fam, n, y) for y in (1, N - 1)]))
    out.append(("random", None, [{k: [rnd.randrange(N) for _ in range(n)] for k in ("aL", "aR", "aO", "sL", "sR")} for _ in range(2)]))
    return out


@pytest.mark.parametrize("n", lz.tcoeffs_lengths())
def test_prover_tcoeffs_on_worst_planes(gpu, n):
    """bpgpu_r1cs_prover_polys / _eval for two provers (y = 1 and y = n - 1) of a circuit with almost no weights, the witness chosen so
    that every plane product of every t-coefficient is the heaviest on the family's indices: t_1..t_6, l_vec, r_vec against model_polys"""
    assert n in (255, 256, 257, 2047, 2048, 2049, 2048 + 256 + 17, 4113)
    rnd = random.Random(n)
    circ = sparse_circuit(n)
    h = gpu.circuit_create(*circ.csr(), circ.n, circ.m)
    nb, np_ = 2, padded(n)
    ys = [1, N - 1]
    zs, xs = [rnd.randrange(N) for _ in range(nb)], [rnd.randrange(N) for _ in range(nb)]
    weights = [cg.model_weights(circ, z) for z in zs]
    assert sum(1 for w in weights[0][:3] for x in w if x) <= 27
    try:
        for name, at, wit in witnesses(n, rnd, lz.TPB):
            col = lambda k: b"".join(le(v) for w in wit for v in w[k])       # noqa: E731
            t, wv, ses = gpu.r1cs_prover_polys(h, nb, n, circ.m, pack(ys), pack([pow(y, -1, N) for y in ys]), pack(zs), col("aL"),
                                               col("aR"), col("aO"), col("sL"), col("sR"))
            try:
                lv, rv = gpu.r1cs_prover_eval(ses, nb, np_, pack(xs))
            finally:
                gpu.prover_destroy(ses)
            for p in range(nb):
                want_t, want_l, want_r = model_polys(circ, weights[p], ys[p], xs[p], wit[p])
                tag = ("prover_tcoeffs", name, at, n, p)
                assert ints(t)[6 * p:6 * p + 6] == want_t, tag
                assert ints(lv)[np_ * p:np_ * (p + 1)] == want_l, tag
                assert ints(rv)[np_ * p:np_ * (p + 1)] == want_r, tag
    finally:
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ the two-party prover's Beaver combines
class Party:
    """One party's run of the two-party prover on one context up to the t-coefficients, on operands chosen by the test: the planes
    of the witness (the same worst witness on the share, MAC and modifier plane), the triples and the OPENED d, e -- which the
    kernels take as given, so that every Beaver term z_k + d y_k + e x_k (+ d e) is the heaviest: x_k = d, y_k = e, d e = C, z_k = C.
    The model of every output is the plain formula of csrc/k_mpc.hip's header on Python integers."""

    def __init__(self, gpu, gens, n, fams, rnd):
        self.gpu, self.n, self.nb = gpu, n, len(fams)
        nb = self.nb
        self.circ = sparse_circuit(n)
        self.ys = [1, N - 1][:nb]
        self.zs = [rnd.randrange(N) for _ in range(nb)]
        self.wit = [lz.tcoeffs_witness(fam, n, y) for fam, y in zip(fams, self.ys)]         # every plane holds this witness
        self.fams = fams
        ops = [b"".join(mont(v) for w in self.wit for _ in range(3) for v in w[k]) for k in ("aL", "aR", "aO", "sL", "sR")]
        self.handle = gpu.circuit_create(*self.circ.csr(), self.circ.n, self.circ.m)
        self.ses = None
        try:
            self.ses, _ = gpu.mpc_prover_commit(gens, None, nb, n, *ops, b"".join(mont(rnd.randrange(N)) for _ in range(9 * nb)))
        except Exception:
            gpu.circuit_destroy(self.handle)
            raise
        # the model's planes: [p][k] -> (l1, l2, l3, r1, r3), and the public r0 [p]
        self.planes, self.r0 = [], []
        for p in range(nb):
            wL, wR, wO = cg.model_weights(self.circ, self.zs[p])[:3]
            y, w = self.ys[p], self.wit[p]
            yp = [pow(y, i, N) for i in range(n)]            # y = +-1: its own inverse
            self.r0.append([(wO[i] - yp[i]) % N for i in range(n)])
            per = []
            for k in range(3):
                mod = k == 2
                per.append(([(w["aL"][i] + (yp[i] * wR[i] if mod else 0)) % N for i in range(n)], w["aO"], w["sL"],
                            [(yp[i] * w["aR"][i] + (wL[i] if mod else 0)) % N for i in range(n)], [yp[i] * w["sR"][i] % N for i in range(n)]))
            self.planes.append(per)

    def close(self):
        if self.ses is not None:
            self.gpu.prover_destroy(self.ses)
        self.gpu.circuit_destroy(self.handle)

    @staticmethod
    def beaver(fam, length, rnd, nprod):
        """per product j: the opened (d, e) lists, worst on the family's indices and 0 elsewhere; the triple is x_k = d, y_k = e, z_k = C
        there and 0 elsewhere, on every plane"""
        out = []
        for _ in range(nprod):
            d, e = lz.beaver_worst(rnd, length)
            hot = [fam.hot(i) for i in range(length)]
            out.append(([x if f else 0 for x, f in zip(d, hot)], [x if f else 0 for x, f in zip(e, hot)], [C if f else 0 for f in hot]))
        return out

    @staticmethod
    def beaver_bytes(bv):
        """-> (triples bytes [p][j][x, y, z][k][i], opened bytes [p][j][d, e][i])"""
        trip = b"".join(b"".join(mont(v) for v in vec) * 3 for prods in bv for d, e, z in prods for vec in (d, e, z))
        opened = b"".join(mont(v) for prods in bv for d, e, _ in prods for vec in (d, e) for v in vec)
        return trip, opened

    @staticmethod
    def beaver_sum(prod, k):
        d, e, z = prod
        return sum(zz + 2 * dd * ee + (dd * ee if k == 2 else 0) for dd, ee, zz in zip(d, e, z)) % N

    def polys(self, rnd):
        """mask + finish -> checks the masked values and t_1..t_6 per plane against the model"""
        gpu, n, nb = self.gpu, self.n, self.nb
        bv = [self.beaver(self.fams[p], n, rnd, 6) for p in range(nb)]
        trip, opened = self.beaver_bytes(bv)
        masked = gpu.mpc_prover_polys_mask(self.ses, self.handle, nb, n, pack(self.ys), pack(self.zs), trip)
        got = [unmont(x) for x in cut(masked, 32)]
        for p in range(nb):
            for j in range(6):
                d, e, _ = bv[p][j]
                for k in range(3):
                    pl = self.planes[p][k]
                    base = ((p * 6 + j) * 2 * 3 + k) * n
                    tag = ("mpc masked", self.fams[p].name, n, p, j, k)
                    assert got[base:base + n] == [(a - x) % N for a, x in zip(pl[j % 3], d)], tag
                    assert got[base + 3 * n:base + 4 * n] == [(a - x) % N for a, x in zip(pl[3 if j < 3 else 4], e)], tag
        t, _, _ = gpu.mpc_prover_polys_finish(self.ses, nb, self.circ.m, opened, b"".join(mont(rnd.randrange(N)) for _ in range(15 * nb)))
        got = [unmont(x) for x in cut(t, 32)]
        ip = lambda a, b: sum(u * v for u, v in zip(a, b)) % N       # noqa: E731
        for p in range(nb):
            for k in range(3):
                l1, l2, l3 = self.planes[p][k][:3]
                P = [self.beaver_sum(bv[p][j], k) for j in range(6)]
                r0 = self.r0[p]
                want = [ip(l1, r0), (P[0] + ip(l2, r0)) % N, (P[1] + ip(l3, r0)) % N, (P[3] + P[2]) % N, P[4], P[5]]
                assert got[(3 * p + k) * 6:(3 * p + k) * 6 + 6] == want, ("mpc_tcoeffs", self.fams[p].name, n, p, k)


@pytest.mark.parametrize("n", lz.mpc_tcoeffs_lengths())
def test_mpc_tcoeffs_on_worst_beaver_terms(gpu, mpc_gens, n):
    """bpgpu_mpc_prover_commit / _polys_mask / _polys_finish for one party of two proofs (y = 1 heaviest throughout, y = n - 1 heaviest
    on the even indices): the masked values and t_1..t_6 on the share, MAC and modifier plane"""
    assert n in (1023, 1024, 1025, 1280 + 17, 2048 + 256 + 3)
    rnd = random.Random(n)
    party = Party(gpu, mpc_gens, n, [lz.Family("worst", n, rnd), lz.Family("worst_even", n, rnd)], rnd)
    try:
        party.polys(rnd)
    finally:
        party.close()


def test_mpc_ipp_combine_folds_twice(gpu, mpc_gens, points):
    """The first round of the shared inner-product argument at padded n = 8192 (h = 4096: 16 trips of k_mpc_ipp_combine, folds on trips
    8 and 16) on one proof whose Beaver terms are all the heaviest: the masked values, and L, R per plane against the oracle's MSM over
    the plane's l(x), r(x), the G / H factors and c_L, c_R from the plain Beaver formula"""
    assert lz.mpc_ipp_lengths() == [8192]
    np_, n = 8192, 4096 + 3
    hh = np_ // 2
    rnd = random.Random(8192)
    party = Party(gpu, mpc_gens, n, [lz.Family("worst", n, rnd)], rnd)
    ipp = None
    try:
        party.polys(rnd)
        x, u, w, y = rnd.randrange(1, N), rnd.randrange(1, N), rnd.randrange(1, N), party.ys[0]
        ipp = gpu.mpc_prover_ipp_begin(party.ses, mpc_gens, np_, n, le(x), le(u), le(w))
        assert gpu.ipp_len(ipp) == np_
        # the model's vectors per plane: l(x), r(x) with the public r0 and the -y^i padding on the modifier plane
        a, b = [], []
        for k in range(3):
            l1, l2, l3, r1, r3 = party.planes[0][k]
            a.append([x * (l1[i] + x * (l2[i] + x * l3[i])) % N for i in range(n)] + [0] * (np_ - n))
            b.append([(x * (r1[i] + x * x * r3[i]) + (party.r0[0][i] if k == 2 else 0)) % N for i in range(n)]
                     + [(-pow(y, i, N)) % N if k == 2 else 0 for i in range(n, np_)])
        fam = lz.Family("worst", hh, rnd)
        bv = [Party.beaver(fam, hh, rnd, 2)]
        trip, opened = Party.beaver_bytes(bv)
        got = [unmont(v) for v in cut(gpu.mpc_ipp_mask(ipp, 1, trip), 32)]
        for j in range(2):
            d, e, _ = bv[0][j]
            for k in range(3):
                base = (j * 2 * 3 + k) * hh
                av, bw = (a[k][hh:], b[k][:hh]) if j else (a[k][:hh], b[k][hh:])
                assert got[base:base + hh] == [(p - q) % N for p, q in zip(av, d)], ("mpc ipp masked d", j, k)
                assert got[base + 3 * hh:base + 4 * hh] == [(p - q) % N for p, q in zip(bw, e)], ("mpc ipp masked e", j, k)
        L, R = gpu.mpc_ipp_round(ipp, 1, opened)
        Gf = [1] * n + [u] * (np_ - n)
        Hf = [pow(y, i, N) * g % N for i, g in enumerate(Gf)]                 # y = 1: y^-i = y^i
        G, H = points[:np_], points[16384:16384 + np_]
        Q = o.point_mul(le(w), o.generator())
        for k in range(3):
            cL, cR = Party.beaver_sum(bv[0][0], k), Party.beaver_sum(bv[0][1], k)
            assert cL == cR == hh * (3 + (k == 2)) * C % N == lz.beaver_plane_sum(hh, k)
            wantL = o.msm(pack([a[k][i] * Gf[hh + i] for i in range(hh)] + [b[k][hh + i] * Hf[i] for i in range(hh)] + [cL]),
                          b"".join(G[hh:] + H[:hh] + [Q]))
            wantR = o.msm(pack([a[k][hh + i] * Gf[i] for i in range(hh)] + [b[k][i] * Hf[hh + i] for i in range(hh)] + [cR]),
                          b"".join(G[:hh] + H[hh:] + [Q]))
            assert L[64 * k:64 * k + 64] == wantL, ("mpc_ipp_combine L", k)
            assert R[64 * k:64 * k + 64] == wantR, ("mpc_ipp_combine R", k)
    finally:
        if ipp is not None:
            gpu.ipp_destroy(ipp)
        party.close()
