"""The inner-product prover's rounds on crafted generators, vectors and challenges (tests/ipp_round_cases.py), bit for bit against
the logarithm model and the CPU oracle.

The prover's operands are the caller's: generators that coincide, are opposite or are the identity, vectors with zero halves, and --
through the stepwise calls -- the challenges.  Random operands never reach the exact cases of the point arithmetic behind
bpgpu_ipp_begin, _begin_gens, _round, _fold, _finish, _folded_gens and _run_fs; these sessions do, at every site the shadow of
ipp_round_cases.py names (tests/test_ipp_round_cases.py holds it to that on the CPU):

  A  sessions over explicit generators, the literal schedule (nb >= 2 with per-proof Q), on the Straus-lane and the bucket route
     1  folds that produce identities at chosen places of k_batch_normalize<8>'s runs (first and second fold, shared and own
        generators), seen through the next rounds' L and R
     2  generators that are multiples of each other inside a fold lane, u = 1
     3  identity input generators: `pinf` lanes, a whole wave with `skip`, zero factors
     4  rounds with zero halves: L or R the identity, an all-zero proof
  B  resident-generator sessions over tables of coinciding generators, c = 8 and 16
     1, 2  k_fixed_msm_ipp<C, 128> (nb = 3) and k_fixed_msm_ipp_g<C> (nb = 8, 9): P + P and P - P in a lane accumulator, in the
        block sum or butterfly, between chunk partial sums; whole MSMs that cancel
     3  rounds 2 and 3 on battery(c) scalars through the hi/lo enumeration, with u = 1 and with the test's own challenges
     4  the fused tail of bpgpu_ipp_run_fs at 2, 3 and 17 partial sums per point, identity L and R absorbed as 64 zero bytes
     5  bpgpu_ipp_folded_gens where the coefficients on coinciding generators cancel or double

Expected points are (sum s_i k_i) B from the model's integers, one oracle scalar multiplication each; where the transcript drives
the challenges they are the oracle's InnerProductProof::create over the same generators.

Deliberately wrong variants of the library, one at a time, against this file and against the suite's earlier prover tests (the tests
of the IPP, the provers, the folds, bpgpu_msm_gens, the window digits, the two-party prover and the host mirror: about 300):
  k_batch_normalize's forward pass without its is_zero_limbs skip: 8 tests here fail (the six fold-identity cases, the multiples
      and the identity inputs); the earlier tests pass
  straus_body's `pinf` bit never set in the fold's two launches (so the product guards and the main loop's guard all see 0; the
      verifier's launches untouched): the same 8 tests fail; the earlier tests pass.  Never set in ANY launch of straus_body and of
      the table kernels: the verifier's earlier tests fail too (154 of them)
  the tail's butterfly without jac_add's out-of-line exact cases, identity selects kept: the three fused-tail tests fail; the earlier
      tests pass
  the tail's strided pass run once: the 17-partial test fails; so do four earlier host-mirror tests (provers with more than 16 chunks)
  (j + 1) % h in the hi/lo enumeration for cur < n0: 19 tests here fail, and 86 earlier ones (any later round of a resident proof)
"""
import pytest

import ipp_round_cases as rc
import oracle_lib as o

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


@pytest.fixture(scope="module")
def tables(gpu):
    """generator tables by (logarithms, c), built once per module: B = B_blinding = the curve generator"""
    made = {}

    def get(cs):
        key = (tuple(cs.kG), tuple(cs.kH), cs.c)
        if key not in made:
            assert cs.shared and cs.kB == 1
            made[key] = gpu.gens_create(rc.pts(cs.kG), rc.pts(cs.kH), o.generator(), o.generator(), cs.c)
        return made[key]
    yield get
    for g in made.values():
        gpu.gens_destroy(g)


def _same_points(got, want, tag):
    assert len(got) == len(want), tag
    if got != want:
        bad = [i for i in range(len(want) // 64) if got[64 * i:64 * i + 64] != want[64 * i:64 * i + 64]]
        raise AssertionError("%s: %d of %d points differ, first at %d (want %s)" % (
            tag, len(bad), len(want) // 64, bad[0], "the identity" if want[64 * bad[0]:64 * bad[0] + 64] == ZERO else "a point"))


def _stepwise(gpu, cs, g=None):
    """the session of `cs` round by round under its own challenges: every round's L and R and the final a, b against the model.
    g: a resident-generator table (else explicit generators).  -> the rounds' (L, R) bytes"""
    nb, n = cs.nb, cs.n
    model = [rc.rounds(cs, p) for p in range(nb)]
    if g is not None:
        s = gpu.ipp_begin_gens(g, nb, n, o.scalars(cs.w), cs.flat(cs.gf), cs.flat(cs.hf), cs.flat(cs.a), cs.flat(cs.b))
    else:
        G = rc.pts(cs.kG) if cs.shared else b"".join(rc.pts(k) for k in cs.kG)
        H = rc.pts(cs.kH) if cs.shared else b"".join(rc.pts(k) for k in cs.kH)
        s = gpu.ipp_begin(nb, n, rc.pts(cs.q), cs.flat(cs.gf), cs.flat(cs.hf), G, H, cs.shared, cs.flat(cs.a), cs.flat(cs.b))
    got = []
    try:
        r = 0
        while gpu.ipp_len(s) > 1:
            L, R = gpu.ipp_round(s, nb)
            _same_points(L, rc.pts([model[p][0][r][0] for p in range(nb)]), "%s round %d L" % (cs.name, r))
            _same_points(R, rc.pts([model[p][0][r][1] for p in range(nb)]), "%s round %d R" % (cs.name, r))
            got.append((L, R))
            gpu.ipp_fold(s, o.scalars(cs.us[r]), o.scalars([rc.inv(u) for u in cs.us[r]]))
            r += 1
        a, b = gpu.ipp_finish(s, nb)
        assert a == o.scalars([m[1] for m in model]) and b == o.scalars([m[2] for m in model]), cs.name
        if g is not None and getattr(cs, "folded", False):
            Gf, Hf = gpu.ipp_folded_gens(s, nb)
            _same_points(Gf, rc.pts([m[0][-1][2][0] for m in model]), cs.name + " folded G")
            _same_points(Hf, rc.pts([m[0][-1][3][0] for m in model]), cs.name + " folded H")
    finally:
        gpu.ipp_destroy(s)
    return got


def _both_routes(gpu, opts, cs):
    """A.5: the round MSMs as Straus lanes and as bucket sums (ipp_pippenger_min lowered: every round has 2 h + 1 >= 3 terms), the same bytes"""
    assert gpu.get_option("ipp_pippenger_min") > 2 * cs.n + 1           # the default keeps these short rounds on the Straus lanes
    want = _stepwise(gpu, cs)
    opts(ipp_pippenger_min=3)
    assert _stepwise(gpu, cs) == want


# ------------------------------------------------------------------ A: explicit generators, literal schedule
@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
@pytest.mark.parametrize("which,n", sorted(rc.FOLD_IDENTITIES), ids=lambda v: str(v))
def test_folds_that_produce_identities_inside_the_normalisation_runs(gpu, opts, which, n, shared):
    """A.1, A.5: nb = 3.  The first (or second) fold gives the identity at the places FOLD_IDENTITIES lists -- first, middle and last in
    a run of k_batch_normalize<8>, a whole run beside a partial one, the short last run (12 lanes) -- for G and, on the second
    stream, for H.  The folded generators show through the following rounds' L and R, where every surviving generator has a
    random scalar: an identity that poisons a neighbour in its run, or is not written as one, changes those bytes."""
    cs = rc.fold_identity_case(which, n, shared)
    _both_routes(gpu, opts, cs)


def test_generators_that_are_multiples_of_each_other_inside_a_fold_lane(gpu, opts):
    """A.2: G_R = G_L, -G_L, 2 G_L (and H likewise) in straus_body<2>'s lanes; proofs 0 and 1 fold with u = 1, so both scalars of a
    lane have the same digits in every window: P + P, P - P and P + 2 P window after window"""
    _both_routes(gpu, opts, rc.multiples_case())


def test_identity_input_generators_a_wave_that_skips_and_lanes_that_do_not(gpu, opts):
    """A.3: nb = 8, n = 32, own generators: the first fold has two waves.  Every left G of wave 0 is the identity (`skip`), wave 1 has
    identity left and right points in single lanes (`pinf`); H mirrors it with the right points of wave 1.  Zero G and H factors."""
    _both_routes(gpu, opts, rc.identity_inputs_case())


@pytest.mark.parametrize("n", [8, 2])
def test_rounds_with_zero_halves_literal(gpu, opts, n):
    """A.4: a_L = 0 and b_R = 0 (L the identity, R ordinary), an all-zero proof, a_R = 0 and b_L = 0; c_L, c_R through Q"""
    cs = rc.zero_halves_case(n)
    want = [rc.rounds(cs, p)[0][0] for p in range(3)]
    assert want[0][0] == 0 and want[0][1] and want[1][:2] == (0, 0) and want[2][1] == 0 and want[2][0]
    _both_routes(gpu, opts, cs)


# ------------------------------------------------------------------ B: resident generators
def test_rounds_with_zero_halves_resident(gpu, tables):
    """A.4 over a table: sc_dot_batched and k_ipp_gens_scalars on all-zero halves (c_L = 0: a zero B scalar)"""
    cs = rc.zero_halves_case(16, shared=True)
    _stepwise(gpu, cs, tables(cs))


@pytest.mark.parametrize("nb", [3, 8])
@pytest.mark.parametrize("c", [8, 16])
def test_coinciding_generators_in_both_round_kernels(gpu, tables, c, nb):
    """B.1, B.2: the first round's L and R of every prover are MSMs picked by the shadow (ipp_round_cases.pair_msms): rows that
    coincide or are opposite meet in a lane accumulator, in the block sum (nb = 3) or the pair-lane butterfly (nb = 8), and as
    equal or opposite chunk partial sums in k_segmented_sum; whole MSMs cancel to 64 zero bytes.  Digits 1, half - 1, -half and
    the top window's.  The later rounds run on under the test's challenges."""
    cases = rc.coinciding_cases(c, nb)
    la = rc.ipp_launch(c, 16, 2 * nb)
    assert (la["grouped"], la["chunks"]) == rc.LAUNCHES[(c, 16, nb)][:2]
    zeros = 0
    for cs in cases:
        got = _stepwise(gpu, cs, tables(cs))
        zeros += sum(1 for side in got[0] for i in range(nb) if side[64 * i:64 * i + 64] == ZERO)
    assert zeros == sum(1 for cs in cases for p in range(nb) for v in rc.rounds(cs, p)[0][0][:2] if v == 0) >= 3


def test_nine_provers_leave_the_first_eight_unchanged(gpu, tables):
    """B.1: nb = 9 is 18 MSMs: the second unit of either side has one live lane (prover 8) and seven clamped to prover 0.  Prover 8's
    L is P + P on row half - 1 and its R is Q - Q; provers 0..7 give the bytes of the nb = 8 session."""
    c = 8
    cs8 = rc.coinciding_cases(c, 8)[0]
    s = rc.one(c, 7, 127)
    cs9 = rc.provers_of(c, rc.pair_msms(c, 8)[:16] + [{1: s, 2: s}, {6: s, 7: s}], 9, 7000)[0]
    cs9.a[:8], cs9.b[:8], cs9.w[:8], cs9.q[:8] = cs8.a, cs8.b, cs8.w, cs8.q
    cs9.us = [r8 + r9[8:] for r8, r9 in zip(cs8.us, cs9.us)]
    assert rc.ipp_launch(c, 16, 18)["chunks"] == 3 and rc.rounds(cs9, 8)[0][0][1] == 0
    g = tables(cs8)
    got8, got9 = _stepwise(gpu, cs8, g), _stepwise(gpu, cs9, g)
    for (L8, R8), (L9, R9) in zip(got8, got9):
        assert L9[:64 * 8] == L8 and R9[:64 * 8] == R8
    assert got9[0][1][64 * 8:] == ZERO


@pytest.mark.parametrize("u_one", [True, False], ids=["u1", "u"])
@pytest.mark.parametrize("nb", [3, 8])
@pytest.mark.parametrize("c", [8, 16])
def test_later_rounds_on_the_battery(gpu, tables, c, nb, u_one):
    """B.3: with u = 1 the coefficients stay 1 and the MSM scalars of rounds 2 and 3 are the folded vectors: battery(c) scalars,
    0 and n - 1, read through the hi/lo enumeration for cur < n0.  With the test's own challenges the same vectors meet coefficients
    that are products of u and u^-1."""
    cs = rc.battery_rounds_case(c, nb, u_one)
    _stepwise(gpu, cs, tables(cs))


def _run_fs(gpu, g, cs):
    """bpgpu_ipp_run_fs over the resident table of `cs`: L, R of every round, the final a, b and the chain states against the
    oracle's InnerProductProof::create over the same generators and the model's transcript"""
    from test_gpu_parity import sys_path_oracle
    sys_path_oracle()
    import pymodel as pm
    nb, n = cs.nb, cs.n
    k = n.bit_length() - 1
    trs = [pm.Transcript(rc.LABEL) for _ in range(nb)]
    for t in trs:
        t.innerproduct_domain_sep(n)
    G, H = rc.pts(cs.kG), rc.pts(cs.kH)
    s = gpu.ipp_begin_gens(g, nb, n, o.scalars(cs.w), cs.flat(cs.gf), cs.flat(cs.hf), cs.flat(cs.a), cs.flat(cs.b))
    try:
        L, R, aa, bb, st = gpu.ipp_run_fs(s, nb, k, b"".join(t.state for t in trs))
    finally:
        gpu.ipp_destroy(s)
    zeros = 0
    for p in range(nb):
        Lo, Ro, ao, bo, ch = o.ipp_create(rc.LABEL, n, rc.pt(cs.q[p]), o.scalars(cs.gf[p]), o.scalars(cs.hf[p]), G, H,
                                          o.scalars(cs.a[p]), o.scalars(cs.b[p]))
        _same_points(L[64 * k * p:64 * k * (p + 1)], Lo, "%s prover %d L" % (cs.name, p))
        _same_points(R[64 * k * p:64 * k * (p + 1)], Ro, "%s prover %d R" % (cs.name, p))
        assert (aa[32 * p:32 * p + 32], bb[32 * p:32 * p + 32]) == (ao, bo), (cs.name, p)
        t = trs[p]
        for r in range(k):
            t.append_message(b"L", Lo[64 * r:64 * r + 64])
            t.append_message(b"R", Ro[64 * r:64 * r + 64])
            assert pm.s2b(t.challenge_scalar(b"u")) == ch[32 * r:32 * r + 32]
            zeros += (Lo[64 * r:64 * r + 64] == ZERO) + (Ro[64 * r:64 * r + 64] == ZERO)
        assert st[32 * p:32 * p + 32] == t.state, (cs.name, p)
    return zeros


@pytest.mark.parametrize("nb", [3, 8])
def test_fused_tail_on_equal_opposite_and_identity_partials(gpu, tables, nb):
    """B.4: the first rounds of B.2 and an all-zero proof through bpgpu_ipp_run_fs: k_ipp_round_tail adds 2 (nb = 3) and 3 (nb = 8)
    partial sums per point -- equal, opposite, identities -- and absorbs an identity L or R as 64 zero bytes"""
    assert rc.ipp_launch(8, 16, 2 * nb)["chunks"] == (2 if nb == 3 else 3)
    zeros = 0
    for cs in rc.coinciding_cases(8, nb) + [rc.zero_proof_case(8, nb)]:
        zeros += _run_fs(gpu, tables(cs), cs)
    assert zeros >= 8 + 3


def test_fused_tail_on_seventeen_partials(gpu, tables):
    """B.4: n0 = cap = 128, nb = 8: 17 partial sums per point, so the tail's strided pass of 16 lanes iterates twice.  Equal (prover 0,
    2) and opposite (1, 2) partials at chunks (0, 16) -- both in lane 0 -- and at (3, 11) -- the butterfly at offset 8; prover 3 is
    all zero."""
    cs = rc.seventeen_chunk_case()
    assert rc.ipp_launch(8, 128, 16)["chunks"] == 17
    assert _run_fs(gpu, tables(cs), cs) >= 2 + 1 + 2 * 7


@pytest.mark.parametrize("c", [8, 16])
def test_folded_generators_that_cancel_or_double(gpu, tables, c):
    """B.5: bpgpu_ipp_folded_gens at n = 1 where the coefficients on the coinciding G_0 = G_8 (H_0 = H_8) are opposite -- the folded
    generator is the identity -- or equal"""
    for cs in rc.folded_gens_cases(c):
        cs.folded = True
        model = [rc.rounds(cs, p)[0][-1] for p in range(cs.nb)]
        assert any(m[2][0] == 0 for m in model) == ("cancel" in cs.name) and all(m[2][0] or m[3][0] for m in model)
        _stepwise(gpu, cs, tables(cs))
