"""The group size of the verifier's two-stage Horner pass (csrc/k_ec.hip: wp_hg, bpgpu_set_horner_group: 8, 16 or 32 windows
per group of the first stage; the second stage then sums 64 / HG partial sums per proof) at every shape the options reach:
whole verifications against the CPU oracle bit for bit, the shapes a pipelined caller's batches take by default against the
short shapes forced, and bpgpu_msm (the same two launchers) on scalars built digit by digit so that the chains start from the
identity, pass through it, and add a point to itself.  Run with `-m gpu` on an MI355X."""
import pytest

import degenerate_cases as dc
import oracle_lib as o
import window_digits as wd
from test_gpu_affine_tables import batches, cat, check_batch, gpu, pool  # noqa: F401  (fixtures and helpers of the same pool)

pytestmark = pytest.mark.gpu
SW, W = 4, 64                      # the window width of the chain and its windows per scalar (csrc/k_ec.hip)
HGS = (8, 16, 32)
assert wd.windows(SW) == W


# ---------------------------------------------------------------- whole verifications
@pytest.mark.parametrize("tnp", [4, 8])
@pytest.mark.parametrize("form", [1, 2], ids=["lane", "quad"])
@pytest.mark.parametrize("hg", HGS)
@pytest.mark.parametrize("nb", [1, 9, 33, 65])
def test_verify_batch_every_shape(gpu, pool, nb, hg, form, tnp):  # noqa: F811
    """Both stages in the form named (groups_form = horner_form: by mode the first stage of these batches would stay on lanes
    whatever the second is forced to).  First-stage chains at HG 32 -- nb = 1: 2; 9: 18, on quads a second block with 2 live
    quads and 14 clamped ones beside the in-place stores; 33: 66, on lanes a second wave with 2 live lanes; 65: the whole pool.
    At HG 8 and 16 nb = 9 gives 72 and 36 chains (5 and 3 blocks of quads, the last one half and a quarter live), nb = 33 gives
    264 and 132 (lanes: 8 and 4 live in the last wave)."""
    with gpu.options(horner_group=hg, horner_form=form, groups_form=form, table_np=tnp):
        oks = [b for recs in batches(pool, nb) for b in check_batch(gpu, pool, recs)]
    assert 0 in oks and 1 in oks


def test_default_route_of_a_pipelined_batch(gpu, pool):  # noqa: F811
    """257 proofs and no option set: the batch takes the shapes of a pipelined caller (not latency mode, nb >= 256).  Same
    outputs as with the short shapes forced (groups of 8, second stage on quads, 4 points per table lane), and both the oracle's."""
    recs = [pool.recs[i % len(pool.recs)] for i in range(257)]
    args = (pool.g, pool.circ, len(recs), pool.n1, pool.k, pool.m, cat(recs, "points"), cat(recs, "scalars"), cat(recs, "challenges"), True, True)
    for name in ("horner_group", "horner_form", "groups_form", "table_np"):
        assert gpu.get_option(name) == 0, name
    by_default = gpu.r1cs_verify_batch(*args)
    with gpu.options(horner_group=8, horner_form=2, table_np=4):
        short = gpu.r1cs_verify_batch(*args)
    assert by_default == short
    oks = check_batch(gpu, pool, recs)
    assert list(oks) == [r.ok for r in recs] and 0 in oks and 1 in oks


# ---------------------------------------------------------------- crafted digits through bpgpu_msm
NPTS = 16                          # one instance of the window-parallel MSM: 64 window sums, then the two Horner stages
FORMS = [(1, 1), (2, 2), (3, 3)]   # (second stage, first stage): a lane, a quad, a wave per chain


def _mul(k, pt):
    return o.point_mul(o.s2b(k % o.N), pt)


@pytest.fixture(scope="module")
def pts():
    """16 points P_j = (j + 2) G and, for P = P_0, the multiples Q_e = 2^e P that a chain meets after e doublings"""
    g = o.generator()
    base = [_mul(j + 2, g) for j in range(NPTS)]
    return dict(base=base, pow={e: _mul(1 << e, base[0]) for e in [4] + [4 * hg for hg in HGS]})


def _scalar(ds):
    s = wd.from_digits(ds, SW)
    assert 0 <= s < o.N and wd.digits(s, SW) == ds, ds
    return s


def _filler(j, lo, hi):
    """non-zero digits for point j in the windows [lo, hi), the highest one positive (so that the scalar is)"""
    ds = [0] * W
    for w in range(lo, hi):
        ds[w] = ((5 * j + 3 * w) % 15) - 7 or 1
    if hi > lo:
        ds[hi - 1] = abs(ds[hi - 1])
    return ds


def _cases(hg, pts):
    """[(name, [(digits, point)] x 16)]: digit vectors over the 64 windows, one per point of the instance"""
    P, zero = pts["base"], [0] * W
    top = W - hg                       # first window of the top group
    out = []
    # (a) every digit of the top group zero: the second stage's chain starts from the identity (and so does every first-stage
    # chain of that group); a second instance leaves the top TWO groups empty
    out.append(("top group zero", [(_filler(j, 0, top), P[j]) for j in range(NPTS)]))
    if W // hg > 2:
        out.append(("top two groups zero", [(_filler(j, 0, top - hg), P[j]) for j in range(NPTS)]))
    # (b) only the top of the scalar non-zero.  At 4-bit windows the top window, 63, starts at bit 252 and n < 2^252: it holds
    # nothing but a carry (wd.top_digit(4) == 0), and a scalar with digit 1 there is below n only with -8 in window 62
    # (2^252 - 2^251).  So: that pair, and the largest digit alone in window 62, the highest window that can stand alone.
    assert wd.top_digit(SW) == 0
    carry = [0] * (W - 2) + [-8, 1]
    out.append(("top window carry", [(carry if j % 3 == 0 else zero, P[j]) for j in range(NPTS)]))
    alone = [0] * (W - 2) + [7, 0]
    out.append(("window 62 alone", [(alone if j in (0, 5) else zero, P[j]) for j in range(NPTS)]))
    # (c) P and -P with the same digits over a whole group (the middle one, or the lower of two): every window sum of the group is
    # the identity and so is its partial sum, an identity addend of the second stage between non-zero groups ...
    g = (W // hg - 1) // 2
    same = _filler(1, g * hg, (g + 1) * hg)
    terms = [(same, P[0]), (same, dc.pt_neg(P[0]))]
    terms += [([d if not g * hg <= w < (g + 1) * hg else 0 for w, d in enumerate(_filler(j, 0, W - 2))], P[j]) for j in range(2, NPTS)]
    out.append(("group cancels", terms))
    # ... and an accumulator that BECOMES the identity: P at window w + 1 and -16 P at window w inside a group; P at the first
    # window of a group and -2^(4 HG) P at the first window of the group below.  Windows further down are non-zero (at HG 32 there are none: the chain ends there).
    for name, hi_w, lo_w, e in (("inside", top + 3, top + 2, 4), ("boundary", top, top - hg, 4 * hg)):
        for sign, tag in ((-1, "acc becomes identity"), (1, "addend equals acc")):      # (d): the same places with +Q -- the doubling case
            Q = pts["pow"][e] if sign > 0 else dc.pt_neg(pts["pow"][e])
            d_hi, d_lo = list(zero), list(zero)
            d_hi[hi_w], d_lo[lo_w] = 1, 1
            terms = [(d_hi, P[0]), (d_lo, Q)] + [(_filler(j, 0, min(lo_w, 5)), P[j]) for j in range(2, NPTS)]
            out.append(("%s, %s" % (tag, name), terms))
    return out


@pytest.mark.parametrize("forms", FORMS, ids=["lane", "quad", "row"])
@pytest.mark.parametrize("hg", HGS)
def test_msm_crafted_digits(gpu, pts, hg, forms):  # noqa: F811
    cases = _cases(hg, pts)
    assert len(cases) == (9 if hg < 32 else 8)          # (two groups at 32: no case with the top two empty)
    with gpu.options(horner_group=hg, horner_form=forms[0], groups_form=forms[1]):
        for name, terms in cases:
            assert len(terms) == NPTS
            sc = b"".join(o.s2b(_scalar(ds)) for ds, _ in terms)
            pt = b"".join(p for _, p in terms)
            assert gpu.msm(sc, pt) == o.msm(sc, pt), (name, hg, forms)


def test_crafted_cases_meet_what_they_claim(pts):
    """on the CPU: the partial sums of the two-stage chain, replayed with the oracle, are the identity / equal where _cases says"""
    for hg in HGS:
        top = W - hg
        cases = dict(_cases(hg, pts))

        def winsum(terms, w):
            sc = b"".join(o.s2b(ds[w] % o.N) for ds, _ in terms)
            return o.msm(sc, b"".join(p for _, p in terms))

        assert all(winsum(cases["top group zero"], w) == dc.IDENT for w in range(top, W))
        g = (W // hg - 1) // 2
        assert all(winsum(cases["group cancels"], w) == dc.IDENT for w in range(g * hg, (g + 1) * hg))
        assert winsum(cases["group cancels"], g * hg - 1 if g else (g + 1) * hg) != dc.IDENT
        for name, hi_w, lo_w, e in (("inside", top + 3, top + 2, 4), ("boundary", top, top - hg, 4 * hg)):
            for tag, equal in (("acc becomes identity", False), ("addend equals acc", True)):
                terms = cases["%s, %s" % (tag, name)]
                acc = _mul(1 << e, winsum(terms, hi_w))          # the accumulator after the doublings between the two windows
                add = winsum(terms, lo_w)
                assert (acc == add) if equal else (acc == dc.pt_neg(add)), (hg, tag, name)
                assert all(winsum(terms, w) == dc.IDENT for w in range(lo_w + 1, W) if w != hi_w)


# ---------------------------------------------------------------- the setting itself
def test_setter_validates(gpu):  # noqa: F811
    """bpgpu_set_horner_group accepts 0, 8, 16, 32 and refuses anything else with BPGPU_E_ARG, leaving the setting as it was"""
    import ctypes as C
    import mpc_bulletproof_amd as m
    old = gpu.get_horner_group()
    try:
        for v in (0, 8, 16, 32):
            gpu.set_horner_group(v)
            assert gpu.get_horner_group() == v == gpu.get_option("horner_group")
        for bad in (-8, -1, 1, 4, 7, 9, 12, 24, 31, 33, 64, (1 << 31) - 1, 1 << 32):
            with pytest.raises(m.BpGpuError) as e:
                gpu.set_horner_group(bad)
            assert e.value.code == m.lib.E_ARG, bad
            assert gpu.get_horner_group() == 32
        lib, w = m.lib._lib, C.c_int(-5)
        assert lib.bpgpu_set_horner_group(None, 8) == m.lib.E_ARG and lib.bpgpu_get_horner_group(None, C.byref(w)) == m.lib.E_ARG
        assert lib.bpgpu_get_horner_group(gpu.ctx, None) == m.lib.E_ARG and w.value == -5
    finally:
        gpu.set_horner_group(old)


def test_environment_seeds_a_new_context_through_the_validator(monkeypatch):
    import mpc_bulletproof_amd as m
    for text, want in (("16", 16), ("32", 32), ("12", 0), ("8x", 0), ("", 0)):
        monkeypatch.setenv("BPGPU_HORNER_GROUP", text)
        g2 = m.BpGpu(0)
        try:
            assert g2.get_horner_group() == want, text
        finally:
            g2.close()
