"""The table walks that fetch a row one addition ahead of its use (csrc/fixed_body.cuh: fixed_chunk_body, fixed_small_body;
csrc/k_ec.hip: k_verify_windows), byte for byte against the CPU oracle on the shapes of tests/table_walk_cases.py:

  generator half   identity generators at the edges of a run, at the end of all and side by side; batches that fill, barely enter and
                   half fill their last wave; runs of 1, 3, 5, 9 generators, the lanes-per-proof walk and latency mode
  k_fixed_msm_m    bpgpu_r1cs_prover_commit with digits that are zero in every lane, in one lane, at both ends of a generator
  window sums      identity points at the edges of the window kernel's 64-point chunks, all but one, all; zero scalars

Expected values are the oracle's (o.msm over the oracle's own scalars, VerifySession); nothing is compared with another GPU result.
Run with `-m gpu` on an MI355X."""
import random
from types import SimpleNamespace

import pytest

import bp_helpers as bh
import oracle_lib as o
import table_walk_cases as tw
import window_digits as wd

pytestmark = pytest.mark.gpu
N = o.N
ZERO = tw.ZERO
LABEL = b"RangeProofTest"


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


def _same_points(got, want, tag):
    assert len(got) == len(want), tag
    if got != want:
        bad = [i for i in range(len(want) // 64) if got[64 * i:64 * i + 64] != want[64 * i:64 * i + 64]]
        raise AssertionError("%s: %d of %d points differ, first at %d" % (tag, len(bad), len(want) // 64, bad[0]))


# ------------------------------------------------------------------ the generator half, a proof per lane and lanes per proof
@pytest.fixture(scope="module")
def pool(gpu):
    """130 proofs of the 8-bit range gadget, three of them tampered, with the oracle's MSM terms of each"""
    recs, cap = bh.make_range_batch(8, max(tw.BATCHES), seed0=5300, tamper={2, 64, 129})
    out = []
    for proof, com in recs:
        s = o.VerifySession(o.K_RANGE, 8, LABEL, [], com, proof, cap)
        k, pts, sc = bh.verify_inputs(proof, com)
        terms_sc, terms_pt = s.msm_terms()
        out.append(SimpleNamespace(points=pts, scalars=sc, challenges=s.challenges(), terms_sc=terms_sc, terms_pt=terms_pt, mega=s.mega_check(),
                                   rc=s.rc))
        dims = SimpleNamespace(n1=s.n1, k=s.k, m=s.m, n=s.n1 + s.n2, nterms=s.nterms, csr=s.csr())
        s.close()
    circ = gpu.circuit_create(*dims.csr, dims.n, dims.m)
    yield SimpleNamespace(recs=out, cap=cap, circ=circ, **{k: v for k, v in vars(dims).items() if k != "csr"})
    gpu.circuit_destroy(circ)


def _cat(recs, key):
    return b"".join(getattr(r, key) for r in recs)


_WANT = {}


def _want_mega(pool, name):
    """the oracle's MSM of every proof's own scalars over the generator list with the identities of set `name`: computed once"""
    if name not in _WANT:
        first = 11 + pool.m              # term of B
        drop = {first + i for i in tw.IDENTITY_SETS[name]}
        _WANT[name] = [o.msm(*tw.drop_terms(r.terms_sc, r.terms_pt, drop)) for r in pool.recs]
    return _WANT[name]


GEN_HALF = [(name, c) for c in (8, 16) for name in ("b_blinding", "chunk_edges", "last_of_all", "consecutive")] + [("combined", 20)]


@pytest.mark.parametrize("name,c", GEN_HALF, ids=["%s-c%d" % p for p in GEN_HALF])
def test_generator_half_with_identity_generators(gpu, opts, pool, name, c):
    """bpgpu_r1cs_verify_batch over generators of which some are the identity (64 zero bytes): such a generator contributes nothing,
    whatever its scalar, at any place of a run.  Every batch size of BATCHES through runs of CHUNK_LENGTHS generators per wave
    (k_verify_back_q: fixed_chunk_body), the lanes-per-proof walk (fixed_chunk_gens = -1) and latency mode (fixed_small_body).
    mega_check against the oracle's MSM of the proof's scalars over the same list, the scalars against the oracle's, the accept
    bit against mega_check == identity.  (c = 20: one table, 7.8 GB, with identities of every kind.)
    At c = 8 the gadget's 18 x 32 (generator, window) pairs are more than one chunk of fixed_msm_chunks, so there the generator half
    is its own chunked launch (k_fixed_msm, which has the identity test too) whatever the option says; the walks of
    fixed_body.cuh run at c = 16 and 20."""
    want = _want_mega(pool, name)
    assert pool.nterms == 36 and all(w != ZERO for w in want)      # no proof verifies against a generator list it was not made for
    assert o.msm(pool.recs[0].terms_sc, pool.recs[0].terms_pt) == pool.recs[0].mega == ZERO      # (o.msm over all terms is mega_check)
    G, H, B, Bb = tw.gens_with_identities(o.gens("G", pool.cap), o.gens("H", pool.cap), o.generator(), o.generator(), tw.IDENTITY_SETS[name])
    g = gpu.gens_create(G, H, B, Bb, c)
    try:
        routes = [("run of %d" % n, dict(fixed_chunk_gens=n), False) for n in tw.CHUNK_LENGTHS]
        routes += [("lanes per proof", dict(fixed_chunk_gens=-1), False), ("latency mode", {}, True)]
        for tag, route, latency in routes:
            opts(fixed_chunk_gens=0)
            opts(**route)
            gpu.set_latency_mode(latency)
            try:
                for nb in tw.BATCHES:
                    recs = pool.recs[:nb]
                    ok, mega, full = gpu.r1cs_verify_batch(g, pool.circ, nb, pool.n1, pool.k, pool.m, _cat(recs, "points"), _cat(recs, "scalars"),
                                                           _cat(recs, "challenges"), True, True)
                    where = "%s c = %d, %s, nb = %d" % (name, c, tag, nb)
                    _same_points(mega, b"".join(want[:nb]), where)
                    assert full == _cat(recs, "terms_sc"), where
                    assert ok == [0] * nb, where
            finally:
                gpu.set_latency_mode(False)
    finally:
        gpu.gens_destroy(g)


def test_generator_half_accepts_over_whole_generators(gpu, opts, pool):
    """the same batches over the generators the proofs were made for: the honest ones are accepted, the tampered ones not"""
    g = gpu.gens_create(o.gens("G", pool.cap), o.gens("H", pool.cap), o.generator(), o.generator(), 8)
    try:
        for n in (3, 5):
            opts(fixed_chunk_gens=n)
            recs = pool.recs[:130]
            ok, mega, _ = gpu.r1cs_verify_batch(g, pool.circ, 130, pool.n1, pool.k, pool.m, _cat(recs, "points"), _cat(recs, "scalars"),
                                                _cat(recs, "challenges"), True, False)
            assert ok == [1 if r.rc == 0 else 0 for r in recs] and ok.count(0) == 3
            _same_points(mega, _cat(recs, "mega"), "run of %d" % n)
    finally:
        gpu.gens_destroy(g)


# ------------------------------------------------------------------ k_fixed_msm_m through bpgpu_r1cs_prover_commit
def _ark(vals):
    return b"".join((v * (1 << 256) % N).to_bytes(32, "little") for v in vals)


@pytest.mark.parametrize("c", [8, 16])
def test_prover_commit_with_zero_digits_at_the_edges_of_a_generator(gpu, c):
    """64 provers of 64 multipliers: k_fixed_msm_m<C> on a (65, 3) grid, two generators per wave (the route of (d) in
    tests/test_gpu_window_digits.py), a prover per lane.  Columns of the witness, that is generators of the table:
      every digit zero in every lane        a_L[3], s_L[7], s_R[7]: the wave fetches no row of that generator
      every digit zero in ONE lane          a_R[10] of prover 21, a_O[11] of prover 63: that lane fetches entry 0 and ignores it
      zero at windows 0, 1, W - 2, W - 1    columns 20 and 21 of a_L, a_O, s_R (an even and an odd generator: both places of a run)
                                            and 62, 63 of a_R, s_L (H_63 is the last generator of all)
      zero at window 0 only                 columns 30, 31: the pair right after a generator boundary
      zero at window W - 1 only             columns 40, 41: the last pair of a generator, of a run where the generator is its second
    every other entry random.  A_I, A_O, S against the oracle's MSMs over [B_blinding, G, H]."""
    nb = n = cap = 64
    W = wd.windows(c)
    rnd = random.Random(900 + c)
    names = ("aL", "aR", "aO", "sL", "sR")
    vec = {nm: [[rnd.randrange(N) for _ in range(n)] for _ in range(nb)] for nm in names}
    ends = (0, 1, W - 2, W - 1)
    seed = 0
    for p in range(nb):
        vec["aL"][p][3] = vec["sL"][p][7] = vec["sR"][p][7] = 0
        for nm, cols in (("aL", (20, 21)), ("aO", (20, 21)), ("sR", (20, 21)), ("aR", (62, 63)), ("sL", (62, 63))):
            for col in cols:
                seed += 1
                vec[nm][p][col] = tw.with_zero_windows(c, ends, seed)
        for nm in names:
            for col, zero in ((30, (0,)), (31, (0,)), (40, (W - 1,)), (41, (W - 1,))):
                seed += 1
                vec[nm][p][col] = tw.with_zero_windows(c, zero, seed)
    vec["aR"][21][10] = 0
    vec["aO"][63][11] = 0
    blinds = [[rnd.randrange(N) for _ in range(3)] for _ in range(nb)]
    flat = lambda rows: [v for r in rows for v in r]      # noqa: E731
    Gp, Hp, B, Bb = o.gens("G", cap), o.gens("H", cap), o.generator(), o.point_mul(o.s2b(0x5DEECE66D), o.generator())
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


# ------------------------------------------------------------------ the window sums
@pytest.fixture(scope="module")
def multi(gpu):
    """ONE proof that 64 values are one bit wide: 87 proof points, two chunks of k_verify_windows; 130 generators, 8-bit tables.
    want[name]: the oracle's MSM of the proof's own scalars with the operands of POINT_PATTERNS[name] left out."""
    param, cap = 1 | (64 << 16), 64
    rc, proof, com = o.r1cs_prove(o.K_RANGE_MULTI, param, LABEL, [(i * 7 >> 2) & 1 for i in range(64)], 6100, cap)
    assert rc == 0
    s = o.VerifySession(o.K_RANGE_MULTI, param, LABEL, [], com, proof, cap)
    assert s.rc == 0 and 11 + s.m + 2 * s.k == tw.NVAR_MULTI
    k, pts, sc = bh.verify_inputs(proof, com)
    terms_sc, terms_pt = s.msm_terms()
    head, ngens = 11 + s.m, 2 + 2 * s.padded_n
    term = [j if j < head else j + ngens for j in range(tw.NVAR_MULTI)]      # operand j of the call is this term of the oracle's list
    assert all(terms_pt[64 * t:64 * t + 64] == pts[64 * j:64 * j + 64] for j, t in enumerate(term))
    want, points = {}, {}
    for name, ids in tw.POINT_PATTERNS.items():
        want[name] = o.msm(*tw.drop_terms(terms_sc, terms_pt, {term[j] for j in ids} | {3, 4, 5}))
        points[name] = b"".join(ZERO if j in ids else pts[64 * j:64 * j + 64] for j in range(tw.NVAR_MULTI))
    assert pts[64 * 3:64 * 6] == ZERO * 3 and want["as_is"] == s.mega_check() == ZERO
    assert sum(1 for w in want.values() if w == ZERO) == 1
    circ = gpu.circuit_create(*s.csr(), s.n1 + s.n2, s.m)
    g = gpu.gens_create(o.gens("G", cap), o.gens("H", cap), o.generator(), o.generator(), 8)
    yield SimpleNamespace(g=g, circ=circ, n1=s.n1, k=s.k, m=s.m, scalars=sc, challenges=s.challenges(), terms_sc=terms_sc, want=want, points=points)
    s.close()
    gpu.gens_destroy(g)
    gpu.circuit_destroy(circ)


@pytest.mark.parametrize("nb", [1, 65])
def test_window_sums_with_identity_points_at_chunk_edges(gpu, multi, nb):
    """the verifier's window-parallel launches (nvar = 87 <= 256) on proofs whose points are the identity as the first point, the
    last of the first chunk, the first of the second, the last of all, four in a row across the chunk boundary, all but one (in
    either chunk: the other chunk has no live point at all) and all.  nb = 1: a call per pattern; nb = 65: the patterns in turn."""
    names = list(tw.POINT_PATTERNS)
    calls = [[nm] for nm in names] if nb == 1 else [[names[i % len(names)] for i in range(nb)]]
    for call in calls:
        ok, mega, full = gpu.r1cs_verify_batch(multi.g, multi.circ, nb, multi.n1, multi.k, multi.m, b"".join(multi.points[nm] for nm in call),
                                               multi.scalars * nb, multi.challenges * nb, True, True)
        _same_points(mega, b"".join(multi.want[nm] for nm in call), "nb = %d, %s" % (nb, call[0]))
        assert ok == [1 if nm == "as_is" else 0 for nm in call]
        assert full == multi.terms_sc * nb


@pytest.mark.parametrize("n", [32, 93])
@pytest.mark.parametrize("nb", [1, 65])
def test_msm_window_parallel_route_with_identity_points_and_zero_scalars(gpu, n, nb):
    """bpgpu_msm / bpgpu_msm_batch below msm_wp_max take the window-parallel launches: one group of 32 points, or six groups of 16
    (the last padded).  Identity points at the edges of a group and side by side, all but one, all; a zero scalar; all scalars
    but one zero.  nb = 1: a call per pattern; nb = 65: the patterns in turn, one MSM each."""
    assert n <= gpu.get_option("msm_wp_max")
    pts = o.gens("G", n)
    pats = tw.msm_patterns(n)
    base = o.unscalars(o.random_scalars(7000 + n, n))
    built = []
    for name, ident, zeros in pats:
        sc = [0 if j in zeros else base[j] for j in range(n)]
        pp = [ZERO if j in ident else pts[64 * j:64 * j + 64] for j in range(n)]
        keep = [j for j in range(n) if j not in ident]
        want = o.msm(o.scalars([sc[j] for j in keep]), b"".join(pp[j] for j in keep)) if keep else ZERO
        built.append((name, o.scalars(sc), b"".join(pp), want))
    assert [b[3] == ZERO for b in built].count(True) == 1
    if nb == 1:
        for name, sc, pp, want in built:
            assert gpu.msm(sc, pp) == want, (n, name)
    else:
        seq = [built[i % len(built)] for i in range(nb)]
        got = gpu.msm_batch(nb, n, b"".join(b[1] for b in seq), b"".join(b[2] for b in seq))
        _same_points(got, b"".join(b[3] for b in seq), "n = %d, nb = %d" % (n, nb))
