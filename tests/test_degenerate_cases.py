"""CPU checks of tests/degenerate_cases.py: the crafted batch that tests/test_gpu_degenerate_points.py feeds to the verification
kernels does reach their exact group-law cases (by the shadow of the kernels' addition order), and the two CPU references --
the C oracle and the Python model -- agree on proofs whose points coincide."""
import os
import sys

import pytest

import degenerate_cases as dc
import oracle_lib as o

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import pymodel as pm   # noqa: E402


@pytest.fixture(scope="module")
def batch():
    return dc.make_batch()


def test_batch_mixes_honest_tampered_and_every_crafted_kind(batch):
    kinds = [r.kind for r in batch]
    assert len(batch) == 70 and kinds.count("tampered") == 1 and kinds.count("honest") >= 20
    assert all(kinds.count(k) >= 4 for k in dc.KINDS)
    assert all(r.ok == 1 for r in batch if r.kind == "honest") and all(r.ok == 0 for r in batch if r.kind == "tampered")
    # role-major lanes, 64 per wave: the first wave of every role holds ordinary and crafted lanes
    assert {"honest"} < set(kinds[:64])
    # no identity point where the transcript validates one: the oracle got as far as the MSM for every proof
    for r in batch:
        assert all(c is not None for c in r.classes[:3] + r.classes[6:]) and r.classes[3:6] == [None] * 3
        assert r.mega != dc.IDENT or r.ok == 1


def test_signed_window_digits_restate_the_device_recoding():
    for s in (0, 1, o.N - 1, 2**251, 0x777 << 240, (0x778 << 240) - 1) + tuple(o.unscalars(o.random_scalars(5, 20))):
        d = dc.digits(s % o.N)
        assert len(d) == 64 and all(-8 <= x <= 7 for x in d) and sum(x << (4 * w) for w, x in enumerate(d)) == s % o.N


def test_every_exact_case_is_reached_at_least_three_times_in_every_order(batch):
    """The condition the GPU tests rest on, for their seeds and batch size: in each Straus lane shape, in the window lanes and in
    the Horner stages the batch meets P + P, P + (-P), an identity accumulator and a doubling of the identity at least 3 times
    (the window lanes never double: three cases there).  Honest proofs meet none of them except the identities of (c)."""
    tot = dc.shadow_batch(batch)
    for od in dc.ORDERS:
        print(od, dict(tot[od]))
    for od in dc.ORDERS:
        for ev in dc.EVENTS:
            if od == "windows" and ev == "dbl0":
                assert tot[od][ev] == 0
            else:
                assert tot[od][ev] >= 3, (od, ev, dict(tot[od]))
    honest = dc.shadow_batch([r for r in batch if r.kind in ("honest", "tampered")])
    for od in dc.ORDERS:
        assert honest[od]["dbl"] == honest[od]["cancel"] == 0
        assert od == "horner" or honest[od]["ident"] == honest[od]["dbl0"] == 0


def test_handful_batches_start_with_a_line_proof(batch):
    first_line = next(r for r in batch if r.kind == "line")
    ev = dc.shadow_all(first_line)
    assert ev["windows"]["dbl"] and ev["windows"]["cancel"] and ev["windows"]["ident"]


@pytest.mark.parametrize("kind", ["twin", "opposite"])
def test_window_shadow_agrees_with_a_direct_digit_comparison(batch, kind):
    """A_I1 and A_O1 are the first two points a window lane adds: with A_O1 = +-A_I1 it meets P + P in the windows where the two
    scalars' digits d, d' satisfy d' = +-d != 0, and P + (-P) where d' = -+d."""
    recs = [r for r in batch if r.kind == kind]
    same = opp = 0
    for r in recs:
        sc = r.var_scalars()
        pairs = list(zip(dc.digits(sc[0]), dc.digits(sc[1])))
        same += sum(1 for a, b in pairs if a == b != 0)
        opp += sum(1 for a, b in pairs if a == -b != 0)
    if kind == "opposite":
        same, opp = opp, same
    tot = dc.shadow_batch(recs)["windows"]
    assert same >= 3 and opp >= 3
    assert tot["dbl"] >= same and tot["cancel"] >= opp and tot["ident"] >= opp


@pytest.mark.parametrize("kind", dc.KINDS)
def test_python_model_and_c_oracle_agree_on_crafted_proofs(batch, kind):
    r = next(x for x in batch if x.kind == kind)
    k, pts11, sc3, L, R, ab = dc.bh.parse_flat_proof(r.proof)
    pt = lambda b, i: pm.b2p(b[64 * i:64 * i + 64])     # noqa: E731
    proof = {nm: pt(pts11, i) for i, nm in enumerate(dc.FIRST11)}
    proof.update(t_x=pm.b2s(sc3[:32]), t_x_blinding=pm.b2s(sc3[32:64]), e_blinding=pm.b2s(sc3[64:]), a=pm.b2s(ab[:32]), b=pm.b2s(ab[32:]),
                 L_vec=[pt(L, j) for j in range(k)], R_vec=[pt(R, j) for j in range(k)])
    ve = pm.Verifier(pm.PedersenGens(), pm.Transcript(dc.LABEL))
    var = ve.commit(pm.b2p(r.com))
    pm.range_proof_gadget(ve, pm.lc_var(var), None, 8)
    scalars, points = ve.verification_msm(proof, pm.BulletproofGens(8))
    assert b"".join(pm.s2b(s) for s in scalars) == r.full
    mega = pm.msm(scalars, points)
    assert pm.p2b(mega) == r.mega
    assert (mega is pm.INF) == (r.ok == 1)


def test_crafted_inner_product_proofs_are_judged_by_the_oracle():
    recs = dc.ipp_batch(4, 5)
    assert [r["kind"] for r in recs] == [None, "twin", "opposite", "line", None]
    assert [r["bit"] for r in recs] == [1, 0, 1, 1, 1]        # the second proof's P is its L_0
    assert all(r["bit_shifted"] == 0 for r in recs)
    r = recs[1]
    assert r["L"] == r["R"] and r["P"] == r["L"][:64] != r["expect"]
    # the model's MSM gives the oracle's expect_P for coinciding L, R
    n, r = 4, recs[2]
    us, uis, s = pm.verification_scalars_from_challenges(o.unscalars(r["ch"]), n)
    a, b = o.unscalars(r["ab"])
    gf, hf = o.unscalars(r["Gf"]), o.unscalars(r["Hf"])
    sc = [a * b] + [a * s[i] * gf[i] for i in range(n)] + [b * s[n - 1 - i] * hf[i] for i in range(n)] + [-x for x in us] + [-x for x in uis]
    pts = [pm.b2p(r[key][64 * i:64 * i + 64]) for key, cnt in (("Q", 1), ("G", n), ("H", n), ("L", 2), ("R", 2)) for i in range(cnt)]
    assert pm.p2b(pm.msm([x % o.N for x in sc], pts)) == r["expect"]
