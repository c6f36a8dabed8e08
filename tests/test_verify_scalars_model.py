"""tests/verify_scalars_model.py against the CPU oracle, before the crafted verifier cases rest on it: for every golden range,
shuffle and example record the model's scalars from VerifySession.csr() and .challenges() are the oracle's msm_terms()[0], its
flattened weights the recorded ones, and the dlog identity the crafted cases use for their expected points gives the oracle's own
mega_check.  No GPU needed."""
import random

import bp_helpers as bh
import oracle_lib as o
import verify_scalars_model as vm

N = vm.N


def H(s):
    return bytes.fromhex(s)


def records(golden_r1cs):
    for rec in golden_r1cs["range"]:
        yield "range", o.K_RANGE, rec["n_bits"], rec, []
    for rec in golden_r1cs["shuffle"]:
        yield "shuffle", o.K_SHUFFLE, rec["k"], rec, []
    for rec in golden_r1cs["example"]:
        yield "example", o.K_EXAMPLE, 0, rec, [rec["values"][5]]


def test_model_scalars_equal_the_oracles_on_the_golden_records(golden_r1cs):
    seen = set()
    for name, kind, param, rec, values in records(golden_r1cs):
        com = b"".join(map(H, rec["commitments"]))
        s = o.VerifySession(kind, param, H(rec["label"]), values, com, H(rec["proof"]), 16)
        try:
            n = s.n1 + s.n2
            csr = s.csr()
            ch = o.unscalars(s.challenges())
            assert len(ch) == 6 + s.k
            wL, wR, wO, wV, wc = vm.flatten(csr, n, s.m, ch[1])
            J = lambda k: o.unscalars(b"".join(map(H, rec[k])))          # noqa: E731
            assert (wL, wR, wO, wV, wc) == (J("wL"), J("wR"), J("wO"), J("wV"), o.b2s(H(rec["wc"]))), name
            k, _, scalars = bh.verify_inputs(H(rec["proof"]), com)
            assert k == s.k
            want, pts = s.msm_terms()
            got = vm.verify_scalars(csr, n, s.n1, s.m, s.k, ch, o.unscalars(scalars))
            assert got == o.unscalars(want), (name, param)
            assert len(got) == s.nterms == vm.nterms(s.m, s.k)
            # the positions the combined checks read: generator columns and proof-point rows partition `full`
            fc, vp = vm.fixed_columns(s.m, s.k), vm.var_positions(s.m, s.k)
            assert sorted(fc + vp) == list(range(s.nterms)) and len(vp) == 11 + s.m + 2 * s.k
            # affine in a: the model at the proof's own a from its values at a = 0 and a = 1
            s0, slope = vm.affine_in_a(csr, n, s.n1, s.m, s.k, ch, o.unscalars(scalars))
            a = o.unscalars(scalars)[3]
            assert [(p + a * q) % N for p, q in zip(s0, slope)] == got
            assert {j for j, q in enumerate(slope) if q} <= {11 + s.m} | set(range(13 + s.m, 13 + s.m + s.padded_n))
            seen.add((name, s.n2 > 0))
        finally:
            s.close()
    assert {nm for nm, _ in seen} == {"range", "shuffle", "example"} and ("shuffle", True) in seen


def test_generator_dlogs_give_the_expected_point():
    """the dlog identity of the crafted cases: with every point a known multiple of the generator, sum scalar * point is
    (sum scalar * dlog) B, one oracle scalar multiplication"""
    rnd = random.Random(8)
    B = o.generator()
    for which in "GH":
        pts, dl = o.gens(which, 5, dlogs=True)
        d = o.unscalars(dl)
        assert all(0 < x < N for x in d) and len(set(d)) == 5
        for i in range(5):
            assert o.point_mul(dl[32 * i:32 * i + 32], B) == pts[64 * i:64 * i + 64], (which, i)
        sc = [rnd.randrange(N) for _ in range(5)]
        assert o.msm(o.scalars(sc), pts) == o.point_mul(o.s2b(sum(s * x for s, x in zip(sc, d))), B)
    assert o.point_mul(o.s2b(0), B) == bytes(64) and o.point_mul(o.s2b(N - 1), B) != bytes(64)


def test_mixed_column_sums_follow_the_common_layout():
    rnd = random.Random(9)
    groups = []
    for m, k, nb in ((1, 1, 3), (2, 2, 2)):
        fulls = [[rnd.randrange(N) for _ in range(vm.nterms(m, k))] for _ in range(nb)]
        groups.append((fulls, [rnd.randrange(1, N) for _ in range(nb)], m, k))
    got = vm.mixed_column_sums(groups)
    assert len(got) == 2 + 2 * 4
    (fa, ra, ma, ka), (fb, rb, mb, kb) = groups
    ca, cb = vm.column_sums(fa, ra, ma, ka), vm.column_sums(fb, rb, mb, kb)
    assert got[0] == (ca[0] + cb[0]) % N and got[1] == (ca[1] + cb[1]) % N
    assert got[2:4] == [(ca[2 + i] + cb[2 + i]) % N for i in range(2)] and got[4:6] == cb[4:6]                  # G: 2 shared, 2 of b alone
    assert got[6:8] == [(ca[4 + i] + cb[6 + i]) % N for i in range(2)] and got[8:10] == cb[8:10]                # H
    assert vm.scaled_var(fa[0], ra[0], ma, ka) == [ra[0] * fa[0][j] % N for j in list(range(12)) + [18, 19]]
