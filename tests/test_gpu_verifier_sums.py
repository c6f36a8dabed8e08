"""The lazy F_n sums of the verifier's scalar assembly on the device, across their fold boundaries, on circuits, challenges and
weights the test chooses (tests/verifier_sum_cases.py: the cases and why; tests/test_verifier_sum_cases.py: the same cases checked
on the CPU; tests/test_lazy_sums_cpu.py: the sites' shapes on a CPU build).  Per-proof calls: every scalar of `full` against
tests/verify_scalars_model.py, mega_check against the expected point and ok against (that point is the identity), on the default
launch route and on a Straus route -- the scalars reach the MSMs through fixed_sc and var_sc, not through `full`, so mega_check is
what shows a wrong store.  Combined calls: the one output point.  All comparisons are byte-exact.

The expected point: every proof point is a known multiple of the generator B, B_blinding is B, and the oracle hands out the
generators' discrete logarithms, so sum scalar * point = (sum scalar * dlog) B: one oracle scalar multiplication.  Proof points
coincide freely; none is the identity.  Every even proof's e_blinding is chosen so that its sum vanishes: those proofs are accepted.
Run with `-m gpu` on an MI355X."""
import random

import pytest

import mpc_dealer as md
import oracle_lib as o
import verifier_sum_cases as vc

pytestmark = pytest.mark.gpu
N = vc.N
le = md.le
IDENT = bytes(64)
CAP = 4096
POOL_DLOGS = list(range(2, 19))       # the proof points: 2 B .. 18 B
VS_LARGE_DEFAULT = 4096               # BPGPU_OPT_VS_LARGE_MIN's default, which the cases' shapes are chosen around
COMBINED_KINDS = ("combined_front_scalars_digits", "combined_sort_accum_reduce", "combined_final")


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    assert g.get_option("vs_large_min") == VS_LARGE_DEFAULT
    yield g
    g.close()


@pytest.fixture
def opts(gpu):
    old = {}

    def set_(**kw):
        for k, v in kw.items():
            old.setdefault(k, gpu.get_option(k))
            gpu.set_option(k, v)
    yield set_
    for k, v in old.items():
        gpu.set_option(k, v)


class Gens:
    def __init__(self, gpu, cap, window_bits):
        G, dG = o.gens("G", cap, dlogs=True)
        H, dH = o.gens("H", cap, dlogs=True)
        self.dG, self.dH = o.unscalars(dG), o.unscalars(dH)
        self.handle = gpu.gens_create(G, H, o.generator(), o.generator(), window_bits)

    def dlogs(self, m, k, point_dlogs):
        """the dlogs of the points of `full`, in its order, for a proof whose own points have point_dlogs"""
        np_ = 1 << k
        assert len(point_dlogs) == 11 + m + 2 * k
        return point_dlogs[:11 + m] + [1, 1] + self.dG[:np_] + self.dH[:np_] + point_dlogs[11 + m:]


@pytest.fixture(scope="module")
def big(gpu):
    """generators for padded_n up to 4096, 4-bit windows (the table stays small; the combined check has no one-stream route for it)"""
    g = Gens(gpu, CAP, 4)
    yield g
    gpu.gens_destroy(g.handle)


@pytest.fixture(scope="module")
def small(gpu):
    """four generators, 8-bit windows: the combined checks' one-stream route"""
    g = Gens(gpu, 4, 8)
    yield g
    gpu.gens_destroy(g.handle)


@pytest.fixture(scope="module")
def pool():
    B = o.generator()
    out, p = [], o.point_add(B, B)
    for _ in POOL_DLOGS:
        out.append(p)
        p = o.point_add(p, B)
    assert out[3] == o.point_mul(le(POOL_DLOGS[3]), B) and len(set(out)) == len(out) and IDENT not in out
    return out


def point_choice(p, nvar):
    """pool indices of proof p's points: they repeat inside a proof and between proofs"""
    return [(5 * p + j) % len(POOL_DLOGS) for j in range(nvar)]


def prepare(case, gens, accepted=lambda p: p % 2 == 0):
    """the operands and expectations of a case's proofs: (scalars bytes, challenges bytes, point indices, full per proof, total per
    proof); every even proof's e_blinding (every proof's that `accepted` names) makes its total vanish"""
    m, k = case.m, case.k
    nvar = 11 + m + 2 * k
    fulls = case.model()
    sc, ch, idx, totals = [], [], [], []
    for p, ((chal, ps), full) in enumerate(zip(case.proofs, fulls)):
        choice = point_choice(p, nvar)
        dl = gens.dlogs(m, k, [POOL_DLOGS[i] for i in choice])
        ps = list(ps)
        if accepted(p):
            rest = sum(s * d for j, (s, d) in enumerate(zip(full, dl)) if j != 12 + m)
            full[12 + m] = -rest % N                                  # B_blinding's scalar -e_blinding - r t_x_blinding
            ps[2] = (rest - chal[5] * ps[1]) % N
            assert (-ps[2] - chal[5] * ps[1]) % N == full[12 + m]
        totals.append(sum(s * d for s, d in zip(full, dl)) % N)
        sc.append(b"".join(le(s) for s in ps))
        ch.append(b"".join(le(c) for c in chal))
        idx.append(choice)
    assert all((t == 0) == accepted(p) for p, t in enumerate(totals)), case.name
    return b"".join(sc), b"".join(ch), idx, fulls, totals


def run_case(gpu, gens, pool, opts, case, routes):
    """one circuit, its proofs, on each route (window-parallel option, through the grid-split kernels or not): full, mega, ok"""
    case.check()
    m, k, nb = case.m, case.k, len(case.proofs)
    sc, ch, idx, fulls, totals = prepare(case, gens)
    pts = b"".join(pool[i] for choice in idx for i in choice)
    want_full = b"".join(le(s) for full in fulls for s in full)
    want_mega = b"".join(o.point_mul(le(t), o.generator()) for t in totals)
    assert want_mega[:64] == IDENT and want_mega[64:128] != IDENT
    h = gpu.circuit_create(*case.csr(), case.n, case.m)
    try:
        for wp, large in routes:
            opts(verify_window_parallel=wp, vs_large_min=1 if large else VS_LARGE_DEFAULT)
            ok, mega, full = gpu.r1cs_verify_batch(gens.handle, h, nb, case.n1, k, m, pts, sc, ch, True, True)
            tag = (case.name, wp, large)
            if full != want_full:
                got = o.unscalars(full)
                bad = [j for j, (a, b) in enumerate(zip(got, o.unscalars(want_full))) if a != b]
                raise AssertionError((tag, "full differs at (proof, position)", [divmod(j, len(fulls[0])) for j in bad[:8]], len(bad)))
            assert mega == want_mega, tag
            assert ok == [1 if t == 0 else 0 for t in totals], tag
    finally:
        gpu.circuit_destroy(h)


DEFAULT_ROUTES = [(1, False), (0, False)]                  # the window-parallel chain, a Straus route
ALL_ROUTES = DEFAULT_ROUTES + [(1, True), (0, True)]       # ... and both again through the grid-split kernels


# ------------------------------------------------------------------------------------------------ the canonical check
@pytest.mark.parametrize("shape", ["fast", "general"])
def test_one_non_canonical_word_rejects_its_proof_on_every_form(gpu, big, pool, opts, shape):
    """Proof 1 of three gets one non-canonical word -- its first or last challenge (y, u_k), its first or last proof scalar (t_x, b);
    the value n or 2^256 - 1 -- on all four routes: the per-proof check inside k_verify_scalars_fast (shape fast) and
    k_verify_scalars (general), and k_scalars_check_proof in front of the grid-split kernels (vs_large_min = 1).  That proof is
    rejected where the unmodified call accepts all three, the other two keep their ok, mega and full, the call succeeds, and the
    context's input flag reads 1, then 0."""
    case = vc.column_case(shape, 1, random.Random("canonical " + shape))
    case.check()
    m, k, nb = case.m, case.k, len(case.proofs)
    assert nb == 3 and case.takes_large_route(1) and not case.takes_large_route()
    sc, ch, idx, fulls, totals = prepare(case, big, accepted=lambda p: True)
    pts = b"".join(pool[i] for choice in idx for i in choice)
    per_full = 32 * len(fulls[0])
    spots = [("challenge", 0), ("challenge", 5 + k), ("scalar", 0), ("scalar", 4)]
    h = gpu.circuit_create(*case.csr(), case.n, case.m)
    try:
        for wp, large in ALL_ROUTES:
            opts(verify_window_parallel=wp, vs_large_min=1 if large else VS_LARGE_DEFAULT)
            ok0, mega0, full0 = gpu.r1cs_verify_batch(big.handle, h, nb, case.n1, k, m, pts, sc, ch, True, True)
            assert ok0 == [1, 1, 1] and gpu.input_flag() == 0
            assert full0 == b"".join(le(s) for full in fulls for s in full)
            for what, j in spots:
                for value in (N, (1 << 256) - 1):
                    bad_sc, bad_ch = bytearray(sc), bytearray(ch)
                    if what == "challenge":
                        bad_ch[32 * ((6 + k) + j):32 * ((6 + k) + j + 1)] = value.to_bytes(32, "little")
                    else:
                        bad_sc[32 * (5 + j):32 * (5 + j + 1)] = value.to_bytes(32, "little")
                    ok, mega, full = gpu.r1cs_verify_batch(big.handle, h, nb, case.n1, k, m, pts, bytes(bad_sc), bytes(bad_ch), True, True)
                    tag = (shape, wp, large, what, j, hex(value))
                    assert ok[1] == 0 and [ok[0], ok[2]] == [ok0[0], ok0[2]], tag
                    for p_ in (0, 2):
                        assert mega[64 * p_:64 * p_ + 64] == mega0[64 * p_:64 * p_ + 64], tag
                        assert full[per_full * p_:per_full * (p_ + 1)] == full0[per_full * p_:per_full * (p_ + 1)], tag
                    assert gpu.input_flag() == 1 and gpu.input_flag() == 0, tag
    finally:
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ the `One` column
@pytest.mark.parametrize("T", vc.one_column_lengths())
@pytest.mark.parametrize("shape", ["fast", "two_phase"])
def test_one_column_across_the_fold(gpu, big, pool, opts, shape, T):
    """w_c over T `One` terms, each product C (and, on the fast shape, n - 1 as a plain value): k_verify_scalars_fast or
    k_verify_scalars by default, k_vsl_wc + k_vsl_tail with vs_large_min = 1 (8, 8, 9 and 17 partials)"""
    assert T in (1023, 1024, 1025, 2065)
    for case in vc.one_column_cases(shape, T):
        assert not case.takes_large_route()
        run_case(gpu, big, pool, opts, case, ALL_ROUTES)


# ------------------------------------------------------------------------------------------------ flatten_column
@pytest.mark.parametrize("shape", ["fast", "general"])
def test_columns_across_flatten_columns_fold(gpu, big, pool, opts, shape):
    """15, 16, 17, 32 and 33 entries in the first and the last live L, R, O column and in V columns: g, h, V_j and delta consume the
    lazy column values"""
    cases = vc.column_cases(shape)
    assert len(cases) == (8 if shape == "fast" else 5)
    for case in cases:
        run_case(gpu, big, pool, opts, case, ALL_ROUTES)


# ------------------------------------------------------------------------------------------------ delta
@pytest.mark.parametrize("ragged", [0, 1])
@pytest.mark.parametrize("padded_n", vc.delta_sizes())
def test_delta_loop_at_its_fold(gpu, big, pool, opts, padded_n, ragged):
    """k_verify_scalars' delta loop with its fold on the last trip (padded_n = 1024) and in mid-loop (2048), every term C, against
    15-entry lazy L columns; n = padded_n and n = padded_n - 3; y = 1, n - 1 and random"""
    assert padded_n in (1024, 2048)
    cases = vc.delta_cases(padded_n)[3 * ragged:3 * ragged + 3]
    for case in cases:
        assert case.n == padded_n - 3 * ragged and not case.takes_large_route()
        run_case(gpu, big, pool, opts, case, DEFAULT_ROUTES)


@pytest.mark.parametrize("ragged", [0, 1])
@pytest.mark.parametrize("padded_n", vc.split_sizes())
def test_delta_through_the_grid_split_kernels(gpu, big, pool, opts, padded_n, ragged):
    """the same circuits through k_vsl_gh + k_vsl_tail: 8, 16 and 32 delta partials, the tail's fold on the last partial and mid-sum"""
    assert padded_n in (1024, 2048, 4096) and vc.split_parts(padded_n) == padded_n // 128
    cases = vc.delta_cases(padded_n)[3 * ragged:3 * ragged + 3]
    for case in cases:
        assert case.takes_large_route(1)
        run_case(gpu, big, pool, opts, case, [(1, True), (0, True)])


# ------------------------------------------------------------------------------------------------ the weighted column sums
def launches(gpu):
    got = {name: cnt for name, (_, cnt) in gpu.profile_read().items() if cnt}
    print(got)
    return got


def group_operands(w, pool):
    nvar = 11 + w.m + 2 * w.k
    choice = point_choice(3, nvar)
    return choice, b"".join(pool[i] for i in choice) * w.nb


# (route, proofs): the one-stream route (verify_combined2_supported) takes at most 65 536 proof points, 4681 of these proofs
WEIGHTED_RUNS = [("one_stream", nb) for nb in vc.weighted_counts() if nb * 14 <= 65536] + [("generic", nb) for nb in vc.weighted_counts()]


@pytest.mark.parametrize("route,nb", WEIGHTED_RUNS)
def test_weighted_column_sums_across_the_fold(gpu, big, small, pool, route, nb):
    """bpgpu_r1cs_verify_combined over nb proofs of a tiny circuit with rho_p = C / s_{p,col} for col = B, G_1 and the last H column:
    comb_colsum_body (8-bit tables, at most 65 536 proof points) and k_sc_weighted_colsum (4-bit tables).  The one-stream route takes
    at most 4681 of these proofs, so its 2 * 4096 + 17 case cannot exist; 4097 is the case that goes on after its fold."""
    assert nb in (4095, 4096, 4097, 8209) and [r for r, _ in WEIGHTED_RUNS].count("one_stream") == 3
    gens = small if route == "one_stream" else big
    gpu.profile_enable(True)
    try:
        for target in vc.WEIGHTED_TARGETS:
            w = vc.weighted(nb, target)
            w.check()
            choice, pts = group_operands(w, pool)
            dl = gens.dlogs(w.m, w.k, [POOL_DLOGS[i] for i in choice])
            want = o.point_mul(le(w.weighted_total(dl)), o.generator())
            h = gpu.circuit_create(*w.csr, w.n, w.m)
            try:
                gpu.profile_read()
                got = gpu.r1cs_verify_combined(gens.handle, h, nb, w.n1, w.k, w.m, pts, w.scalar_bytes(), w.challenge_bytes(), w.rho_bytes())
                ran = launches(gpu)
            finally:
                gpu.circuit_destroy(h)
            # which column sum ran: the one-stream route reports its stages under the combined kinds, the generic one does not
            assert [ran.get(kd, 0) for kd in COMBINED_KINDS] == ([1, 1, 1] if route == "one_stream" else [0, 0, 0]), (route, ran)
            assert got == want and got != IDENT, (route, nb, target)
    finally:
        gpu.profile_enable(False)


@pytest.mark.parametrize("target", vc.MIXED_TARGETS, ids=lambda t: t if t == "B" else "%s%d" % t)
def test_mixed_column_sums_cross_the_fold_in_the_second_segment(gpu, small, pool, target):
    """bpgpu_r1cs_verify_mixed_combined over 2049 proofs of padded_n = 2 and 2050 of padded_n = 4: lane 0's counter reaches its fold
    inside the second segment; G_3 and H_3 take terms from the second segment alone"""
    groups = vc.mixed(target)
    assert [g.nb for g in groups] == [2049, 2050]
    handles, args, total = [], [], 0
    gpu.profile_enable(True)
    try:
        for w in groups:
            w.check()
            choice, pts = group_operands(w, pool)
            total += w.weighted_total(small.dlogs(w.m, w.k, [POOL_DLOGS[i] for i in choice]))
            h = gpu.circuit_create(*w.csr, w.n, w.m)
            handles.append(h)
            args.append(dict(circuit=h, nb=w.nb, n1=w.n1, k=w.k, points=pts, scalars=w.scalar_bytes(), challenges=w.challenge_bytes(),
                             rho=w.rho_bytes()))
        gpu.profile_read()
        got = gpu.r1cs_verify_mixed_combined(small.handle, args)
        ran = launches(gpu)
        assert [ran.get(kd, 0) for kd in COMBINED_KINDS] == [1, 1, 1], ran        # the mixed queue's launches (k_mix_k1 among the first)
        assert got == o.point_mul(le(total % N), o.generator()) and got != IDENT, target
    finally:
        gpu.profile_enable(False)
        for h in handles:
            gpu.circuit_destroy(h)
