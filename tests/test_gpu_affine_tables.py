"""The table launch of the verifier (csrc/k_ec.hip: {1..8} P of every proof point, built in affine coordinates with one shared
inversion per level at 4 and 8 points per lane, by the Jacobian chain at 1 and 2) and the window sums that read the tables, on
batches that mix honest proofs, scalar-tampered proofs and proofs some of whose points are the identity encoding -- at other
positions in every such proof, so that the identity masks of the table lanes differ inside a wave at every lane shape.  Accept
bits, mega_check points (of rejected proofs too) and MSM scalars must be the CPU oracle's, bit for bit.  The 8-bit range gadget:
18 proof points, a multiple of neither 4 nor 8.  Run with `-m gpu` on an MI355X."""
import random
from types import SimpleNamespace

import pytest

import degenerate_cases as dc
import oracle_lib as o

pytestmark = pytest.mark.gpu
NVAR = 18
# The reference's transcript rejects an identity in most slots before any MSM, so the oracle's session has no mega_check for such
# a proof.  The C ABI takes points, scalars and challenges side by side, though: the identity encodings go into the POINTS of a
# proof whose scalars and challenges are the honest replay's, and the expected mega_check is the oracle's MSM over the session's
# own terms with the same points replaced.  The scalars are unchanged; the sum loses s_v P_v, so the proof is rejected.
FREE = [v for v in range(NVAR) if v not in (3, 4, 5)]      # A_I2, A_O2, S2 are the identity already (one-phase proof)
NB_MAX = 65


def with_identities(rec, positions):
    """overwrite the proof points `positions` (operand order) of an honest Rec with the identity encoding"""
    sc, pts = rec.terms
    head = 11 + rec.m
    pts = bytearray(pts)
    points = bytearray(rec.points)
    for v in positions:
        t = v if v < head else rec.nterms - 2 * rec.k + (v - head)      # the term of operand v (degenerate_cases.Rec.var_scalars)
        assert bytes(pts[64 * t:64 * t + 64]) == bytes(points[64 * v:64 * v + 64]) != dc.IDENT
        pts[64 * t:64 * t + 64] = dc.IDENT
        points[64 * v:64 * v + 64] = dc.IDENT
    rec.points, rec.mega, rec.ok = bytes(points), o.msm(sc, bytes(pts)), 0
    assert rec.mega != dc.IDENT


def make_pool():
    """65 proofs: honest, identity-crafted and scalar-tampered in turn; every identity-crafted proof has another non-empty set of
    positions (the 15 single positions first, then sets of 2 to 6)"""
    rnd = random.Random(4242)
    patterns = [(v,) for v in FREE] + [tuple(sorted(rnd.sample(FREE, rnd.randrange(2, 7)))) for _ in range(NB_MAX)]
    rnd.shuffle(patterns)
    recs = []
    for i in range(NB_MAX):
        seed = 3000 + i
        v = (0x9E3779B97F4A7C15 * (seed + 1)) % (1 << 8)
        rc, proof, com = o.r1cs_prove(o.K_RANGE, 8, dc.LABEL, [v], seed, 8)
        assert rc == 0
        kind = ("honest", "identity", "tampered")[i % 3]
        if kind == "tampered":
            proof = dc.tamper_scalar(proof, seed)
        r = dc.Rec(kind, proof, com, None, 8, 8)
        r.ident = ()
        assert r.nvar == NVAR and r.ok == (0 if kind == "tampered" else 1)
        if kind == "identity":
            s = o.VerifySession(o.K_RANGE, 8, dc.LABEL, [], com, proof, 8)
            r.terms = s.msm_terms()
            s.close()
            assert o.msm(*r.terms) == r.mega == dc.IDENT
            r.ident = patterns[i // 3]
            with_identities(r, r.ident)
        recs.append(r)
    return recs


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def pool(gpu):
    recs = make_pool()
    r0 = recs[0]
    circ = gpu.circuit_create(*r0.csr, r0.n, r0.m)
    g = gpu.gens_create(o.gens("G", 8), o.gens("H", 8), o.generator(), o.generator(), 8)
    yield SimpleNamespace(recs=recs, circ=circ, g=g, n1=r0.n1, k=r0.k, m=r0.m)
    gpu.gens_destroy(g)
    gpu.circuit_destroy(circ)


def test_identity_masks_differ_inside_a_wave(pool):
    """the premise of the batches below, checked on the operand order alone: at every lane shape some table lane (role r holds
    the points r + j * lanes) sees other identity masks in different proofs of the first 22"""
    for tnp in (1, 2, 4, 8):
        lanes = (NVAR + tnp - 1) // tnp
        differing = 0
        for r in range(lanes):
            masks = set()
            for rec in pool.recs[:22]:
                pts = rec.points
                masks.add(tuple(pts[64 * v:64 * v + 64] == dc.IDENT for v in range(r, NVAR, lanes)))
            differing += len(masks) > 1
        assert differing >= 2, tnp


def cat(recs, key):
    return b"".join(getattr(r, key) for r in recs)


def check_batch(gpu, pool, recs):
    nb = len(recs)
    ok, mega, full = gpu.r1cs_verify_batch(pool.g, pool.circ, nb, pool.n1, pool.k, pool.m, cat(recs, "points"), cat(recs, "scalars"),
                                           cat(recs, "challenges"), True, True)
    for i, r in enumerate(recs):
        assert ok[i] == r.ok, (i, r.kind, r.ident)
        assert mega[64 * i:64 * i + 64] == r.mega, (i, r.kind, r.ident)
        assert full[32 * r.nterms * i:32 * r.nterms * (i + 1)] == r.full, (i, r.kind, r.ident)
    return ok


def batches(pool, nb):
    """the first nb proofs of the pool (honest, identity, tampered, ...).  One proof cannot be accepted and rejected: nb = 1 is
    three batches of one, an honest, an identity-crafted and a tampered proof."""
    return [[r] for r in pool.recs[:3]] if nb == 1 else [pool.recs[:nb]]


ROUTES = [dict(table_np=t) for t in (1, 2, 4, 8)] + [dict()]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: "tnp=%d" % r["table_np"] if r else "default")
@pytest.mark.parametrize("nb", [1, 3, 22, 65])
def test_verify_batch(gpu, pool, nb, route):
    """22 proofs x 3 lanes (8 points per lane) and 65 x 5 lanes (4 per lane) cross a wave boundary and leave clamped lanes"""
    old = gpu.get_option("table_np")
    gpu.set_option("table_np", route.get("table_np", 0))
    try:
        oks = [b for recs in batches(pool, nb) for b in check_batch(gpu, pool, recs)]
    finally:
        gpu.set_option("table_np", old)
    assert 0 in oks and 1 in oks


@pytest.mark.parametrize("nb", [1, 3, 22, 65])
def test_verify_batch_latency_mode(gpu, pool, nb):
    gpu.set_latency_mode(True)
    try:
        oks = [b for recs in batches(pool, nb) for b in check_batch(gpu, pool, recs)]
    finally:
        gpu.set_latency_mode(False)
    assert 0 in oks and 1 in oks


@pytest.mark.parametrize("n", [1, 9, 100])
def test_msm_entry_point(gpu, n):
    """bpgpu_msm through the same table and window launches: repeated points, P beside -P, identity points (100 terms run as
    7 instances of 16 points, the last one padded with identities)"""
    rnd = random.Random(500 + n)
    base = [o.point_mul(o.s2b(rnd.randrange(1, o.N)), o.generator()) for _ in range(max(1, n // 3))]
    pts = []
    for i in range(n):
        p = base[i % len(base)]                       # every point several times
        pts.append(dc.IDENT if n > 1 and i % 7 == 3 else (dc.pt_neg(p) if i % 5 == 4 else p))
    sc = [rnd.randrange(o.N) for _ in range(n)]
    if n >= 9:
        sc[1] = sc[1 + len(base)] if 1 + len(base) < n else sc[1]       # s P + s P, and s P + s (-P) where the signs differ
        sc[2] = 0
        sc[5] = o.N - 1
    scb, ptb = b"".join(o.s2b(s) for s in sc), b"".join(pts)
    assert gpu.msm(scb, ptb) == o.msm(scb, ptb)
    if n > 1:          # every term cancels against its twin: the sum is the identity
        twin = b"".join(dc.pt_neg(p) for p in pts)
        assert gpu.msm(scb + scb, ptb + twin) == dc.IDENT == o.msm(scb + scb, ptb + twin)
