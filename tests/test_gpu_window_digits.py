"""Every signed-window MSM kernel on scalars built digit by digit (tests/window_digits.py), bit for bit against the CPU oracle.

Each MSM kernel recodes a scalar into digits in [-half, half - 1], half = 2^(c-1), and a digit indexes a row of a fixed-base table
page or a bucket.  Magnitude `half` occurs only as the negative extreme and selects the LAST row of a page, row
(g W + w) half + half - 1, which the last lane of the table fill's last run writes; a random window is there with probability
2^-c, so a test on random scalars reads that row, its neighbour half - 1 and both signs of them at c = 16 or 20 only if it pushes
tens of thousands of scalars through one table (the host mirror's generator derivation does, at c = 16; no MSM, table or verifier
test did).  Here every such digit sits in every window of every kernel:

  (a) bpgpu_generator_mul (k_fixed_single<16>, the derivation of every Bulletproofs generator)
  (b) bpgpu_msm_gens at every table width on every launch shape of launch_fixed reachable with kinds = 0
  (c) the same with generators that coincide, so that a table walk meets P + P and P - P in a lane accumulator, a butterfly or a
      block sum
  (d) the MSM-per-lane commitment kernel (k_fixed_msm_m, kinds = 3) through bpgpu_r1cs_prover_commit
  (e) the first round of the resident-generator IPP (k_fixed_msm_ipp, k_fixed_msm_ipp_g)
  (f) the variable-base routes: window-parallel launches, Straus lanes, k_pip.hip at c = 8, 10, 11, 13, 15 and k_pip2.hip

The generator half of the verifier (fixed_small_body<C, 64>, fixed_chunk_body with AHEAD > 1) takes scalars derived from the
transcript's challenges: they cannot be crafted, and there is no entry point that would feed it others.  It runs the bodies of
csrc/fixed_body.cuh that (b) to (d) run with chosen digits.

Many MSMs use generators k_i G with known k_i, so the expected point is (sum s_i k_i) G: one scalar multiplication of the oracle.
"""
import random

import pytest

import oracle_lib as o
import pip_shapes
import window_digits as wd
from test_gpu_parity import _pip_points, _pip_want, pip_base      # noqa: F401  (pip_base: the module-scoped fixture of the bucket-route tests)

pytestmark = pytest.mark.gpu
N = o.N
ZERO = bytes(64)


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture
def opts(gpu):
    """set launch-route options of the shared context for ONE test (bpgpu_set_option); the previous values come back afterwards"""
    old = {}

    def set_(**kw):
        for k, v in kw.items():
            old.setdefault(k, gpu.get_option(k))
            gpu.set_option(k, v)
    yield set_
    for k, v in old.items():
        gpu.set_option(k, v)


def _mulG(k):
    return o.point_mul(o.s2b(k), o.generator())


def _neg(pt):
    return pt[:32] + ((o.P - int.from_bytes(pt[32:], "little")) % o.P).to_bytes(32, "little")


def _same_points(got, want, tag):
    """got == want, 64 bytes at a time, naming the first point that differs"""
    assert len(got) == len(want), tag
    if got != want:
        bad = [i for i in range(len(want) // 64) if got[64 * i:64 * i + 64] != want[64 * i:64 * i + 64]]
        raise AssertionError("%s: %d of %d points differ, first at %d" % (tag, len(bad), len(want) // 64, bad[0]))


def _ark(vals):
    return b"".join((v * (1 << 256) % N).to_bytes(32, "little") for v in vals)


# ------------------------------------------------------------------ (a) bpgpu_generator_mul
def test_generator_mul_on_the_16_bit_battery(gpu):
    """k_fixed_single<16>: one lane per scalar over the context's table of the curve generator.  battery(16) has -2^15 (the last
    row of a page), 2^15 - 1, +-1 and -(2^15 - 1) in each of the 15 lower windows and 1, 2, 2047, 2048 in the top one.  One call
    of all of them, and one of 1 000 scalars: 15 full blocks of 64 lanes and one of 40."""
    rnd = random.Random(1601)
    bat = wd.battery(16)
    sc = list(bat.values()) + [0, 1, N - 1] + [rnd.randrange(N) for _ in range(50)]
    want = {s: _mulG(s) for s in sc}
    assert want[0] == ZERO
    _same_points(gpu.generator_mul(o.scalars(sc)), b"".join(want[s] for s in sc), "battery(16) + edges")
    big = [sc[(7 * i) % len(sc)] for i in range(1000)]
    assert len(big) % 64 and set(big) == set(sc)
    _same_points(gpu.generator_mul(o.scalars(big)), b"".join(want[s] for s in big), "1000 scalars")


# ------------------------------------------------------------------ (b), (c) bpgpu_msm_gens
def _launch_shapes(gpu, g, n, msms, ks, seed, tag):
    """msms: scalar lists of 2 + 2n entries over generators k_i G.  Every MSM through the three launch shapes that launch_fixed
    (csrc/k_fixed.hip) has for one chunk and (2 + 2n) W <= 16 384 pairs:
      nb < 64           k_fixed_msm<C, 128>, a block per MSM         (calls of at most 63)
      64 <= nb < 1024   k_fixed_msm_small<C, 32>, two MSMs per wave  (calls of at most 1 023, a short one padded to 64)
      nb >= 1024        k_fixed_msm_small<C, 16>, four MSMs per wave (one call, padded to 1 024)
    The padding is random MSMs, checked like the rest."""
    per = 2 + 2 * n
    assert all(len(m) == per for m in msms) and len(ks) == per

    def point(m):
        return _mulG(sum(s * k for s, k in zip(m, ks)) % N)
    want = [point(m) for m in msms]
    npad = max(64, 1024 - len(msms))
    flat = o.unscalars(o.random_scalars(seed, npad * per))
    pads = [flat[per * i:per * (i + 1)] for i in range(npad)]
    padw = [point(m) for m in pads]

    def call(ms, ws, shape):
        got = gpu.msm_gens(g, len(ms), n, o.scalars([s for m in ms for s in m]))
        _same_points(got, b"".join(ws), "%s %s nb = %d" % (tag, shape, len(ms)))
    for i in range(0, len(msms), 63):
        call(msms[i:i + 63], want[i:i + 63], "block")
    for i in range(0, len(msms), 1023):
        k = max(0, 64 - len(msms[i:i + 1023]))
        call(msms[i:i + 1023] + pads[:k], want[i:i + 1023] + padw[:k], "small32")
    k = max(0, 1024 - len(msms))
    call(msms + pads[:k], want + padw[:k], "small16")
    return want


KB = 0x5DEECE66D1234567890ABCDEF0FEDCBA9876543210F00DFACE       # the discrete logarithm of the B_blinding of these tests


@pytest.mark.parametrize("c", [4, 8, 10, 12, 14, 16, 20])
def test_msm_gens_every_table_width_on_every_launch_shape(gpu, c):
    """A table of capacity 1 -- B, B_blinding, G_0, H_0, all distinct -- at every width bpgpu_gens_create accepts (c = 20: 13 pages
    of 2^19 rows per generator, 1.7 GB).  battery(c) in MSMs of 4 scalars, each four in its 4 rotations, so every battery scalar
    meets every generator.  Route (fixed_msm_chunks, launch_fixed): total = 4 W <= 256 pairs, so by_work = ceil(total / 512) = 1
    and chunks = 1 at any nb; kinds = 0 rules the MSM-per-lane kernel out; chunks == 1 and total <= 16 384 leave the choice to nb
    alone, as _launch_shapes lists it (bpgpu_msm_gens passes lpm = 0)."""
    (G0, dg), (H0, dh) = o.gens("G", 1, dlogs=True), o.gens("H", 1, dlogs=True)
    ks = [1, KB, o.b2s(dg), o.b2s(dh)]
    bat = list(wd.battery(c).values())
    bat += [0] * (-len(bat) % 4)
    msms = [bat[j:j + 4][r:] + bat[j:j + 4][:r] for j in range(0, len(bat), 4) for r in range(4)]
    assert 64 <= len(msms) < 1024
    g = gpu.gens_create(G0, H0, o.generator(), _mulG(KB), c)
    try:
        _launch_shapes(gpu, g, 1, msms, ks, 2000 + c, "c = %d" % c)
    finally:
        gpu.gens_destroy(g)


@pytest.mark.parametrize("c", [8, 16])
def test_msm_gens_chunked_launch_with_partial_sums(gpu, c):
    """Capacity 16, n = 16, nb = 2: total = 34 W pairs (1 088 at c = 8, 544 at c = 16), by_work = ceil(total / 512) = 3 and 2,
    by_fill = 512, so chunks = 3 and 2: k_fixed_msm<C, 128> on a (chunks, 2) grid into partial sums, then segmented_sum.  The
    battery is laid over all 34 generators, call after call, each call one scalar further round."""
    cap = n = 16
    (Gp, dg), (Hp, dh) = o.gens("G", cap, dlogs=True), o.gens("H", cap, dlogs=True)
    ks = [1, KB] + o.unscalars(dg) + o.unscalars(dh)
    bat = list(wd.battery(c).values())
    per = 2 + 2 * n
    g = gpu.gens_create(Gp, Hp, o.generator(), _mulG(KB), c)
    try:
        for k in range(-(-len(bat) // (2 * per))):
            flat = [bat[(2 * per * k + i) % len(bat)] for i in range(2 * per)]
            flat = flat[k % per:] + flat[:k % per]
            want = b"".join(_mulG(sum(s * kk for s, kk in zip(flat[per * b:per * (b + 1)], ks)) % N) for b in range(2))
            _same_points(gpu.msm_gens(g, 2, n, o.scalars(flat)), want, "c = %d call %d" % (c, k))
    finally:
        gpu.gens_destroy(g)


@pytest.mark.parametrize("c", [8, 16])
def test_msm_gens_coinciding_generators_inside_the_table_walks(gpu, c):
    """Capacity 2 with B = B_blinding = G_0 = H_0 = P and G_1 = -H_1 = Q: generators [P, P, P, Q, P, -Q].  Per MSM two generators
    that coincide get one non-zero digit in the same window w and every other digit of the MSM is zero, for every pair of them
    (six among the four P, and Q with -Q), every w < W - 1 and, for `same`, the top window too:
      same      the digit d on both, d in 1, half - 1, -half (a negative d with its +1 in window w + 1): P + P on rows d, also on the
                last row of the page, wherever the two rows are added; on Q, -Q the same digits give Q - Q there.  In the top
                window d is 1 and t, the largest digit whose value is below n (8 at c = 8, 2 048 at c = 16)
      opposite  d on the first and -d, with +1 in window w + 1, on the second, d in 1, half - 1: P - P in window w, the row of window
                w + 1 remains; on Q, -Q it is Q + Q.  (+half is no digit, so -half has no opposite: its P - P is `same` on Q, -Q)
    Where they are added: 6 W pairs (192 at c = 8, 96 at c = 16) make one chunk, so _launch_shapes' three kernels run.  A lane of
    the block kernel takes pairs l, l + 128: B and H_0 are 4 W = 128 pairs apart at c = 8 and share a lane (xyzz_madd), the others
    meet in the block sum.  The 16-lane kernel strides by 16, which divides W = 32 and 16: every pair meets in a lane accumulator
    (xyzz_madd_nzq).  The 32-lane kernel strides by 32: the same at c = 8, but at c = 16 generators g and g + 1 sit in lanes w and
    w + 16, so the pairs an odd distance apart -- (0, 1), (1, 2), (1, 4) -- meet in the shuffle butterfly (jac_add) and the others
    in a lane.  Also whole MSMs that cancel: 64 zero bytes."""
    W, half = wd.windows(c), 1 << (c - 1)
    p, q = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA998877, 0x7A6B5C4D3E2F10213243546576879809A0B1C2D3E4F5
    P, Q = _mulG(p), _mulG(q)
    ks = [p, p, p, q, p, N - q]
    pairs = [(0, 1), (0, 2), (0, 4), (1, 2), (1, 4), (2, 4), (3, 5)]
    tops = sorted({1, wd.top_digit(c)})
    assert len(tops) == 2

    def one(w, d):
        return (d << (c * w)) + ((1 << (c * (w + 1))) if d < 0 else 0)
    msms = []
    for i, j in pairs:
        for w in range(W - 1):
            for d in (1, half - 1, -half):
                m = [0] * 6
                m[i] = m[j] = one(w, d)
                assert wd.digits(m[i], c)[w] == d
                msms.append(m)
            for d in (1, half - 1):
                m = [0] * 6
                m[i], m[j] = one(w, d), one(w, -d)
                assert wd.digits(m[j], c)[w] == -d and wd.digits(m[j], c)[w + 1] == 1
                msms.append(m)
        for d in tops:
            m = [0] * 6
            m[i] = m[j] = d << (c * (W - 1))
            assert m[i] < N and wd.digits(m[i], c)[W - 1] == d
            msms.append(m)
    first = len(msms)
    rnd = random.Random(77 + c)
    bat = list(wd.battery(c).values())
    for s in bat[::7] + [rnd.randrange(1, N) for _ in range(8)]:       # whole MSMs that cancel
        a, b = rnd.choice(bat), rnd.randrange(N)
        msms += [[s, N - s, 0, 0, 0, 0], [0, 0, s, 0, N - s, 0], [0, 0, 0, s, 0, s], [s, a, b, 0, (3 * N - s - a - b) % N, 0],
                 [s, 0, N - s, a, 0, a]]
    g = gpu.gens_create(P + Q, P + _neg(Q), P, P, c)
    try:
        want = _launch_shapes(gpu, g, 2, msms, ks, 3000 + c, "c = %d" % c)
        assert all(w == ZERO for w in want[first:])
        # Q - Q under equal digits leaves the identity; P - P under opposite digits leaves the row of window w + 1
        assert sum(1 for w in want[:first] if w == ZERO) == 3 * (W - 1) + len(tops)
    finally:
        gpu.gens_destroy(g)


# ------------------------------------------------------------------ (d) the MSM-per-lane commitment kernel
@pytest.mark.parametrize("c", [8, 16])
def test_prover_commit_per_lane_kernel_on_the_battery(gpu, c):
    """bpgpu_r1cs_prover_commit with nb = 64 provers of n = 64 multipliers: 192 MSMs of kinds = 3 classes, so fixed_per_lane
    (kinds > 0, nb >= 64 kinds, n >= 64) holds; fixed_per_lane_gens gives sets = 1, target = 1 024, ceil(130 / 1 024) = 1 -> 2
    generators per chunk, 65 chunks: k_fixed_msm_m<C> on a (65, 3) grid, fixed_chunk_body<C, 1>, then segmented_sum.  A wave is the
    64 provers' MSMs of one class over two generators, window after window.  (The c = 16 table of 130 generators is 4.4 GB.)
    Every operand is a battery(c) scalar, except three columns that are zero but for ONE prover's single-digit scalar: in that
    digit's window one lane of the wave adds and 63 do not, in the generator's other windows no lane does -- the wave-uniform
    skips of the kernel.  A_I, A_O, S against the oracle's MSMs over [B_blinding, G, H]."""
    nb = n = cap = 64
    W, half = wd.windows(c), 1 << (c - 1)
    bat = list(wd.battery(c).values())
    named = wd.battery(c)
    Gp, Hp, B, Bb = o.gens("G", cap), o.gens("H", cap), o.generator(), _mulG(KB)
    vec = {}
    for k, nm in enumerate(("aL", "aR", "aO", "sL", "sR")):
        vec[nm] = [[bat[(5 * (p * n + i) + k + p) % len(bat)] for i in range(n)] for p in range(nb)]
    assert {s for v in vec.values() for row in v for s in row} == set(bat)
    lone = (("aL", 5, 17, "w3:1"), ("aO", 40, 63, "w%d:%d" % (W - 2, -half)), ("sR", 63, 0, "w0:%d" % (half - 1)))
    for nm, col, lane, case in lone:
        for p in range(nb):
            vec[nm][p][col] = named[case] if p == lane else 0
    blinds = [[bat[(3 * p + k) % len(bat)] for k in range(3)] for p in range(nb)]
    flat = lambda rows: [v for r in rows for v in r]      # noqa: E731
    g = gpu.gens_create(Gp, Hp, B, Bb, c)
    ses = None
    try:
        ses, got = gpu.r1cs_prover_commit(g, None, nb, n, _ark(flat(vec["aL"])), _ark(flat(vec["aR"])), _ark(flat(vec["aO"])),
                                          _ark(flat(blinds)), s_L=_ark(flat(vec["sL"])), s_R=_ark(flat(vec["sR"])))
        want = b""
        for p in range(nb):
            want += o.msm(o.scalars([blinds[p][0]] + vec["aL"][p] + vec["aR"][p]), Bb + Gp + Hp)
            want += o.msm(o.scalars([blinds[p][1]] + vec["aO"][p]), Bb + Gp)
            want += o.msm(o.scalars([blinds[p][2]] + vec["sL"][p] + vec["sR"][p]), Bb + Gp + Hp)
        _same_points(got, want, "c = %d: A_I, A_O, S of 64 provers" % c)
    finally:
        if ses is not None:
            gpu.prover_destroy(ses)
        gpu.gens_destroy(g)


# ------------------------------------------------------------------ (e) the first round of the resident-generator IPP
@pytest.mark.parametrize("nb", [3, 8])
@pytest.mark.parametrize("c", [8, 16])
def test_ipp_resident_generators_first_round_on_the_battery(gpu, c, nb):
    """bpgpu_ipp_begin_gens with G and H factors all 1: the scalars of the first round's L and R MSMs (k_ipp_gens_scalars) are the
    witness entries themselves, and these are battery(c) scalars (8 provers of n = 16 hold all of them).  nb = 3 is 6 MSMs:
    ipp_grouped (nmsm >= 16) is false, k_fixed_msm_ipp<C, 128>; nb = 8 is 16 MSMs: k_fixed_msm_ipp_g<C>, a wave of 8 MSMs x 8
    pair-lanes.  L, R of every round and the final a, b against the oracle's InnerProductProof::create."""
    from test_gpu_parity import _ipp_create_gpu, sys_path_oracle
    sys_path_oracle()
    n = cap = 16
    bat = list(wd.battery(c).values())
    a = o.scalars([bat[i % len(bat)] for i in range(nb * n)])
    b = o.scalars([bat[(nb * n + i) % len(bat)] for i in range(nb * n)])
    if nb == 8:
        assert set(o.unscalars(a + b)) == set(bat)
    ones = o.scalars([1] * (nb * n))
    w = o.random_scalars(450 + c, nb)
    Gp, Hp, B = o.gens("G", cap), o.gens("H", cap), o.generator()
    g = gpu.gens_create(Gp, Hp, B, _mulG(KB), c)
    try:
        Ls, Rs, aa, bb, _ = _ipp_create_gpu(gpu, b"innerproducttest", nb, n, None, ones, ones, None, None, True, a, b, gens=g, w=w)
        for p in range(nb):
            sl = slice(32 * n * p, 32 * n * (p + 1))
            Q = o.point_mul(w[32 * p:32 * p + 32], B)
            L, R, ao, bo, _ = o.ipp_create(b"innerproducttest", n, Q, ones[sl], ones[sl], Gp, Hp, a[sl], b[sl])
            assert (Ls[p], Rs[p], aa[32 * p:32 * p + 32], bb[32 * p:32 * p + 32]) == (L, R, ao, bo), p
    finally:
        gpu.gens_destroy(g)


# ------------------------------------------------------------------ (f) the variable-base routes
def _dispatch(gpu, n):
    """the route of a one-instance bpgpu_msm of n terms under the context's options, as msm_batch_dev_locked (csrc/bpgpu_api.hip)
    chooses it: a default that moves (msm_wp_max 2^15, pippenger_min 512, msm_pip2_single 0) then fails the test"""
    wp_max, pip_min, pip2 = (gpu.get_option(k) for k in ("msm_wp_max", "pippenger_min", "msm_pip2_single"))
    if n <= wp_max:
        return "window_parallel"
    if pip2 and pip_min <= n and 1 << 8 <= n <= 1 << 16:
        return "k_pip2"
    return "k_pip" if n >= pip_min else "straus_lanes"


# (route, plan row of tests/pip_shapes.py or None, n, options)
VARIABLE_BASE = [
    ("window_parallel", None, 2048, {}),                                       # the default route up to 2^15 terms
    ("straus_lanes", None, 2048, dict(msm_wp_max=0, pippenger_min=4096)),       # below pippenger_min: the 4-bit Straus lanes
    ("k_pip_c8", None, 2048, dict(msm_wp_max=0)),
    ("k_pip2", None, 4096, dict(msm_wp_max=0, msm_pip2_single=1)),
    ("k_pip_c10", "A", None, dict(msm_wp_max=0)),
    ("k_pip_c11", "skewed40037", None, {}),
    ("k_pip_c13_two_level", "C", None, dict(msm_wp_max=0)),
    ("k_pip_c15", "E", None, {}),
]


@pytest.mark.parametrize("route,row,n,options", VARIABLE_BASE, ids=[v[0] for v in VARIABLE_BASE])
def test_variable_base_routes_on_all_widths(gpu, opts, pip_base, route, row, n, options):      # noqa: F811
    """all_widths() -- the batteries of all twelve widths, so the test need not know the route's -- in the leading terms of an MSM
    over the points of the bucket-route tests (identities, duplicates and P / -P pairs among them; the crafted scalars skip the
    identity points), once with every other scalar zero, so that the crafted digits are alone in their buckets, and once with
    random ones.  Against MSM(s_i, k_i G) = (sum s_i k_i) G.  Shape F of pip_shapes.py (c = 16, 737 400 terms) is left out: preparing
    its operands on the host takes longer than a test of a few seconds may, and E runs the same kernels of the two-level sort."""
    import mpc_bulletproof_amd as m
    if row is not None:
        _, n = pip_shapes.assert_plan(row)
    elif route == "k_pip_c8":
        assert m.lib.pippenger_plan(1, n)["c"] == 8
    opts(**options)
    assert _dispatch(gpu, n) == ("k_pip" if route.startswith("k_pip_c") else route)
    pts, dl = _pip_points(pip_base, n)
    crafted = wd.all_widths()
    at = [i for i in range(n) if pts[64 * i:64 * i + 64] != ZERO][:len(crafted)]
    assert len(at) == len(crafted) and at[-1] < 2048
    for fill in (bytes(32 * n), o.random_scalars(9000 + n, n)):
        sc = bytearray(fill)
        for i, s in zip(at, crafted):
            sc[32 * i:32 * i + 32] = o.s2b(s)
        sc = bytes(sc)
        assert gpu.msm(sc, pts) == _pip_want(sc, dl), (route, "zero fill" if fill[:64] == ZERO else "random fill")
