"""CPU checks of tests/ipp_round_cases.py: the sessions that tests/test_gpu_ipp_round_cases.py drives do reach the exact group-law
cases at every site the shadow names, the launch shapes the placements rely on are the ones csrc/k_fixed.hip computes, the identity
placements sit where they claim inside k_batch_normalize's runs, and the logarithm model agrees with the C oracle's
InnerProductProof::create on generators that coincide."""
import ctypes as C
import os
import re
import subprocess

import pytest

import ipp_round_cases as rc
import oracle_lib as o
import window_digits as wd

HERE = os.path.dirname(os.path.abspath(__file__))
K_FIXED = os.path.join(os.path.dirname(HERE), "mpc_bulletproof_amd", "csrc", "k_fixed.hip")
N = o.N


@pytest.fixture(scope="module")
def cover():
    return rc.coverage()


# ------------------------------------------------------------------ launch shapes
@pytest.fixture(scope="module")
def chunks_fn():
    """ipp_grouped and fixed_msm_ipp_chunks, cut out of csrc/k_fixed.hip (plain host C++) and compiled as they stand"""
    src = open(K_FIXED).read()
    grouped = re.search(r"^static bool ipp_grouped\(size_t nmsm\) \{.*?\}", src, re.M)
    chunks = re.search(r"^size_t fixed_msm_ipp_chunks\(int c, size_t n0, size_t nmsm\) \{.*?^\}", src, re.M | re.S)
    assert grouped and chunks, "fixed_msm_ipp_chunks has moved: re-derive ipp_round_cases.ipp_launch and LAUNCHES from the new code"
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    cpp, so = os.path.join(out, "ipp_chunks.cpp"), os.path.join(out, "libipp_chunks.so")
    text = "#include <cstddef>\n" + grouped.group(0) + "\nextern \"C\" " + chunks.group(0) + "\n"
    if not os.path.exists(cpp) or open(cpp).read() != text or not os.path.exists(so):
        with open(cpp, "w") as f:
            f.write(text)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, cpp])
    lib = C.CDLL(so)
    lib.fixed_msm_ipp_chunks.restype = C.c_size_t
    lib.fixed_msm_ipp_chunks.argtypes = [C.c_int, C.c_size_t, C.c_size_t]
    return lib.fixed_msm_ipp_chunks


def test_launch_shapes_are_the_ones_the_placements_assume(chunks_fn):
    for (c, n0, nb), (grouped, chunks, per, cases) in rc.LAUNCHES.items():
        got = chunks_fn(c, n0, 2 * nb)
        msg = "c = %d, n0 = %d, nb = %d: %%s -- re-place: %s" % (c, n0, nb, cases)
        assert got == chunks, msg % ("fixed_msm_ipp_chunks gives %d chunks, the cases assume %d" % (got, chunks))
        la = rc.ipp_launch(c, n0, 2 * nb)
        assert (la["grouped"], la["chunks"], la["per"]) == (grouped, chunks, per), msg % ("the shadow's launch is %r" % (la,))
    # the shadow's copy of the heuristic follows the source over every shape near the ones used
    for c in (4, 8, 16):
        for n0 in (2, 16, 32, 128, 1024):
            for nmsm in (2, 6, 14, 16, 18, 64, 512):
                assert rc.ipp_launch(c, n0, nmsm)["chunks"] == chunks_fn(c, n0, nmsm), (c, n0, nmsm)
    # the numbers the issue quotes
    assert [rc.LAUNCHES[k][1] for k in ((8, 16, 3), (8, 16, 8), (8, 128, 8))] == [2, 3, 17] and rc.LAUNCHES[(8, 16, 8)][2] == 184
    assert (1 + 128) * 32 == 4128


def test_lane_strides_and_pair_rounding_as_in_the_source():
    """what ipp_launch and shadow_msm copy from launch_fixed_ipp and the two kernels, expression by expression (the chunk COUNTS are
    held by the compiled function above): if one of these moves, the shadow's lanes are no longer the kernels' and every placement of
    ipp_round_cases.py has to be looked at again.  Compared without white space, so a reformatted line still matches."""
    def squeeze(text):          # spacing, line breaks and the casts' spelling do not matter: only the tokens do
        return re.sub(r"\s+", "", text).replace("(size_t)", "")
    src = squeeze(open(K_FIXED).read())
    for line in ("per = (total + chunks - 1) / chunks;",                           # pairs per chunk ...
                 "per = (per + 7) & ~7;",                                          # ... a multiple of the pair-lanes in the grouped kernel
                 "(k_fixed_msm_ipp<C, 128>), dim3(chunks, nmsm), dim3(128)",       # lane stride 128, a block per (chunk, MSM)
                 "PL = 8;",                                                        # lane stride 8
                 "for (int off = 8; off < 64; off <<= 1)",                         # butterfly offsets 8, 16, 32
                 "(j / h) * cur + (use_hi ? h : 0) + j % h;"):                     # the hi/lo enumeration
        assert squeeze(line) in src, "csrc/k_fixed.hip no longer has `%s`: re-derive the shadow (ipp_round_cases.shadow_msm)" % line
    tail = squeeze(open(os.path.join(os.path.dirname(K_FIXED), "k_transcript.hip")).read())
    for line in ("for (size_t i = ll; i < chunks; i += 16)",                        # the tail's stride of 16 ...
                 "for (int off = 8; off > 0; off >>= 1)"):                         # ... and its butterfly offsets 8, 4, 2, 1
        assert squeeze(line) in tail, "csrc/k_transcript.hip no longer has `%s`: re-derive ipp_round_cases.shadow_tail" % line


# ------------------------------------------------------------------ every (site, event) the design names
@pytest.mark.parametrize("kernel", ["block", "grouped"])
def test_both_msm_kernels_meet_every_exact_case_at_every_site(cover, kernel):
    ev = cover[kernel]
    for site in ("lane", "reduce", "partials"):
        for e in ("dbl", "cancel", "ident"):
            assert ev.count(site, e) >= 2, (kernel, site, e)
    assert ev.count("partials", "zero_out") >= 2
    assert ev.identity_partials("partials") >= 2        # identity partial sums, not the lanes that hold nothing


@pytest.mark.parametrize("chunks", [2, 3, 17])
def test_the_fused_tail_meets_every_exact_case(cover, chunks):
    ev = cover["tail%d" % chunks]
    for e in rc.EVENTS:
        assert ev.count("tail", e) >= 2, (chunks, e)
    # `ident` above also counts the butterfly's empty lanes: these are identity partial sums in the strided pass itself
    assert ev.identity_partials("tail") >= 2, chunks


def test_seventeen_chunks_equal_pairs_meet_where_they_claim(cover):
    """chunks (0, 16): lane 0's second strided iteration; chunks (3, 11): the butterfly at offset 8, lane 3"""
    cs = rc.seventeen_chunk_case()
    la = rc.ipp_launch(8, 128, 16)
    assert [rc.chunk_of(la, t, w) for t in (1, 125, 24, 86) for w in (0, 31)] == [0, 0, 16, 16, 3, 3, 11, 11], \
        "the 17-chunk layout moved: re-place seventeen_chunk_case's terms 1, 125, 24, 86"
    res = rc.Resident(cs)
    ev = rc.Events()
    L0 = rc.shadow_msm(res.terms(0)[0], la, ev)
    R0 = rc.shadow_msm(res.terms(0)[1], la, ev)
    assert L0[0] == L0[16] != 0 and [i for i, v in enumerate(L0) if v] == [0, 16]
    assert R0[3] == R0[11] != 0 and [i for i, v in enumerate(R0) if v] == [3, 11]
    where = cover["tail17"].where
    assert ("tail", "dbl", ("stride", 0, 1)) in where and ("tail", "cancel", ("stride", 0, 1)) in where
    assert ("tail", "dbl", ("bfly", 8, 3)) in where and ("tail", "cancel", ("bfly", 8, 3)) in where
    # prover 1: L and R are the identity; prover 3: every partial is
    _, lr = rc.shadow_resident_round(res, la, tail=True)
    assert lr[1] == (0, 0) and lr[3] == (0, 0) and all(lr[0]) and lr[2][0] != 0 and lr[2][1] == 0


def test_fold_lanes_meet_every_exact_case_and_a_wave_skips(cover):
    ev = cover["fold"]
    for e in rc.EVENTS:
        assert ev.count("fold_lane", e) >= 2, e
    cs = rc.identity_inputs_case()
    G, H = rc.gens_before_round(cs, 0)
    assert rc.shadow_fold(cs, 0, "G", G)[2] == [(True, False), (False, False)]        # wave 0: every left point; wave 1: mixed
    assert rc.shadow_fold(cs, 0, "H", H)[2] == [(False, False), (False, True)]
    for side, k in (("G", G), ("H", H)):
        mixed = [[k[p][j * 16 + i] == 0 for p in rng for i in range(16)] for j in (0, 1) for rng in (range(4), range(4, 8))]
        assert sum(1 for m in mixed if any(m) and not all(m)) >= 2, side           # `pinf` lanes next to ordinary ones
    assert any(f == 0 for row in cs.gf for f in row) and any(f == 0 for row in cs.hf for f in row)
    # A.2: with u = 1 and factors 1 both scalars of a lane are 1, the same digits in every window
    cs = rc.multiples_case()
    assert rc.fold_lane_scalars(cs, 0, 0, 1, "G", 4) == (1, 1)
    s = rc.fold_lane_scalars(cs, 0, 1, 2, "H", 4)
    assert s[0] == s[1] != 1
    out = rc.shadow_fold(cs, 0, "G", rc.gens_before_round(cs, 0)[0])[1]
    assert out[1] == 0 and out[0] == 2 * cs.kG[0][0] % N and out[2] == 3 * cs.kG[0][2] % N        # G_R = -G_L, G_L, 2 G_L


# ------------------------------------------------------------------ A.1: the identity placements
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("which,n", sorted(rc.FOLD_IDENTITIES))
def test_fold_identities_land_at_the_run_positions_they_claim(which, n, shared):
    cs = rc.fold_identity_case(which, n, shared)
    r = 0 if which == "first" else 1
    h = n >> (r + 1)
    total = cs.nb * h
    assert total == {("first", 16): 24, ("first", 8): 12, ("later", 16): 12}[(which, n)]
    for side, idx in (("G", 2), ("H", 3)):
        flat = [rounds_p[r][idx][i] for rounds_p in (rc.rounds(cs, p)[0] for p in range(cs.nb)) for i in range(h)]
        assert [f for f, v in enumerate(flat) if v == 0] == sorted(cs.placed[side]), (side, "the fold's identities are not where listed")
        # ... and the fold lanes' own walk gives the same points
        before = rc.gens_before_round(cs, r)[0 if side == "G" else 1]
        assert rc.shadow_fold(cs, r, side, before)[1] == flat
        # no input generator and no factor became zero on the way
        assert all(v for p in range(cs.nb) for v in cs.gens_of(p)[idx - 2]) and all(v for row in (cs.gf if side == "G" else cs.hf) for v in row)
    want = {("first", 16): ({"first", "middle", "last", "whole", "whole_next_to_partial"}, {"middle", "whole", "whole_next_to_partial"}),
            ("first", 8): ({"middle", "first", "last", "short"}, {"first", "last", "whole", "whole_next_to_partial", "short"}),
            ("later", 16): ({"first", "middle", "last", "short"}, {"middle", "whole", "whole_next_to_partial", "short"})}[(which, n)]
    assert (rc.run_positions(cs.placed["G"], total), rc.run_positions(cs.placed["H"], total)) == want
    if shared:
        assert all(len(set(row)) == 1 for row in cs.us)


def test_fold_identities_cover_every_placement_on_both_sides():
    for side in "GH":
        got = set()
        for (which, n), placed in rc.FOLD_IDENTITIES.items():
            got |= rc.run_positions(placed[side], 3 * (n // (2 if which == "first" else 4)))
        assert got == {"first", "middle", "last", "whole", "whole_next_to_partial", "short"}, side
    assert 3 * 4 % 8 != 0        # nb h of the short-run shapes is no multiple of 8


# ------------------------------------------------------------------ the model against the oracle
def _oracle(cs, p):
    kG, kH = cs.gens_of(p)
    n = cs.n
    return o.ipp_create(rc.LABEL, n, rc.pt(cs.q[p]), o.scalars(cs.gf[p]), o.scalars(cs.hf[p]), rc.pts(kG), rc.pts(kH),
                        o.scalars(cs.a[p]), o.scalars(cs.b[p]))


@pytest.mark.parametrize("make", [rc.zero_halves_case, rc.multiples_case, lambda: rc.fold_identity_case("first", 8, False),
                                  lambda: rc.coinciding_cases(8, 3)[0], lambda: rc.zero_proof_case(8, 3)],
                         ids=["zero_halves", "multiples", "fold_identities", "coinciding", "zero_proof"])
def test_logarithm_model_agrees_with_the_oracle_under_its_challenges(make):
    """InnerProductProof::create of the C oracle over the crafted generators; the model replays it with the oracle's challenges"""
    cs = make()
    k = cs.n.bit_length() - 1
    for p in range(cs.nb):
        L, R, a, b, ch = _oracle(cs, p)
        for r in range(k):
            cs.us[r][p] = o.b2s(ch[32 * r:32 * r + 32])
        rr, am, bm = rc.rounds(cs, p)
        assert L == rc.pts([x[0] for x in rr]) and R == rc.pts([x[1] for x in rr]), (cs.name, p)
        assert (a, b) == (o.s2b(am), o.s2b(bm)), (cs.name, p)
    if cs.name == "zero_halves":
        rr = [rc.rounds(cs, p)[0] for p in range(3)]
        assert rr[0][0][0] == 0 and rr[0][0][1] != 0 and rr[2][0][1] == 0 and rr[2][0][0] != 0
        assert all(x[0] == 0 and x[1] == 0 for x in rr[1])


# ------------------------------------------------------------------ the resident bookkeeping
@pytest.mark.parametrize("u_one", [True, False])
@pytest.mark.parametrize("nb", [3, 8])
def test_resident_terms_sum_to_the_folded_rounds_and_carry_the_battery(nb, u_one):
    c = 8
    cs = rc.battery_rounds_case(c, nb, u_one)
    res = rc.Resident(cs)
    bat = set(wd.battery(c).values()) | {0, N - 1}
    seen = set()
    for r in range(4):
        for p in range(nb):
            want = rc.rounds(cs, p)[0][r]
            Lt, Rt = res.terms(p)
            assert (sum(s * k for s, k in Lt) % N, sum(s * k for s, k in Rt) % N) == want[:2], (r, p)
            # the generator the MSM kernel reads for a term is the one whose coefficient the scalars kernel multiplied in
            if u_one and r in (1, 2):
                sc = {s for s, _ in Lt[1:] + Rt[1:]}
                assert sc <= bat, (r, p)
                seen |= sc
        res.fold(cs.us[r])
    if u_one:
        assert {0, N - 1} <= seen and len(seen) >= (20 if nb == 3 else 60)
    for p in range(nb):
        assert (res.a[p][0], res.b[p][0]) == rc.rounds(cs, p)[1:]


def test_coinciding_cases_lay_the_picked_msms_out_as_first_rounds():
    for c, nb in ((8, 3), (8, 8), (16, 3), (16, 8)):
        msms = rc.pair_msms(c, 3 if nb < 8 else 8)
        cases = rc.coinciding_cases(c, nb)
        half, ds = 1 << (c - 1), set()
        for m in msms:
            for s in m.values():
                ds |= set(wd.digits(s, c))
        assert {1, half - 1, -half, wd.top_digit(c)} <= ds, (c, nb)
        flat = []
        for cs in cases:
            res = rc.Resident(cs)
            for p in range(nb):
                for terms in res.terms(p):
                    flat.append({t: s for t, (s, _) in enumerate(terms) if s and t})
                    assert [k for _, k in terms[1:]] == rc.coinciding_table(c)[0][1:]
        assert flat[:len(msms)] == [dict(m) for m in msms]


def test_folded_gens_cases_cancel_and_double():
    for c in (8, 16):
        can, dbl = rc.folded_gens_cases(c)
        for cs, want_g in ((can, (0, 0, 1)), (dbl, (1, 1, 1))):
            res = rc.Resident(cs)
            for r in range(4):
                res.fold(cs.us[r])
            for p in range(3):
                g, h = res.folded_gens(p)
                assert (g != 0) == bool(want_g[p]), (cs.name, p)
                assert (g, h) == tuple(x[0] for x in rc.rounds(cs, p)[0][3][2:])
                if want_g[p]:
                    assert g == 2 * res.cG[p][0] * rc.KP % N
            assert [res.folded_gens(p)[1] == 0 for p in range(3)] == ([False, False, True] if cs is can else [False] * 3)
