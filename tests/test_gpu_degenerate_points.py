"""The verifier's variable-base MSM routes on proofs whose points coincide (tests/degenerate_cases.py): duplicates, opposite pairs,
all points on one line, proof points that are resident generators -- mixed with honest and scalar-tampered proofs in one batch.
Such inputs make the kernels' additions meet P + P, P + (-P) and identity accumulators (tests/test_degenerate_cases.py proves,
on the CPU, that this batch does so in every addition order), cases honest proofs never reach.  Every route must give the CPU
oracle's accept bits, mega_check points and MSM scalars, bit for bit.  Run with `-m gpu` on an MI355X."""
import random
from types import SimpleNamespace

import pytest

import degenerate_cases as dc
import oracle_lib as o

pytestmark = pytest.mark.gpu
NVAR = 18      # proof points of the 8-bit range gadget: 11 + m + 2k, m = 1, k = 3


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


def cat(recs, key):
    return b"".join(getattr(r, key) for r in recs)


@pytest.fixture(scope="module")
def batch(gpu):
    """the 70 crafted proofs with the oracle's verdicts, the circuit and the generators (capacity 8, 8-bit table windows)"""
    recs = dc.make_batch()
    r0 = next(r for r in recs if r.kind == "honest")
    circ = gpu.circuit_create(*r0.csr, r0.n, r0.m)
    g = gpu.gens_create(o.gens("G", 8), o.gens("H", 8), o.generator(), o.generator(), 8)
    first = [next(i for i, r in enumerate(recs) if r.kind == k) for k in ("line", "honest", "twin", "opposite", "gens", "line_B", "tampered")]
    rest = [i for i in range(len(recs)) if i not in first]
    yield SimpleNamespace(recs=recs, circ=circ, g=g, n1=r0.n1, k=r0.k, m=r0.m, order=first + rest)
    gpu.gens_destroy(g)
    gpu.circuit_destroy(circ)


def pick(batch, nb):
    """all 70 proofs in their shuffled order, or nb < 70 of them: a `line` proof, an honest one, then one of every other kind"""
    return batch.recs if nb == len(batch.recs) else [batch.recs[i] for i in batch.order[:nb]]


def check_batch(gpu, batch, recs):
    nb = len(recs)
    ok, mega, full = gpu.r1cs_verify_batch(batch.g, batch.circ, nb, batch.n1, batch.k, batch.m, cat(recs, "points"), cat(recs, "scalars"),
                                           cat(recs, "challenges"), True, True)
    for i, r in enumerate(recs):
        assert ok[i] == r.ok, (i, r.kind)
        assert mega[64 * i:64 * i + 64] == r.mega, (i, r.kind)
        assert full[32 * r.nterms * i:32 * r.nterms * (i + 1)] == r.full, (i, r.kind)
    assert 0 in ok and (1 in ok or nb == 1)


WP = [dict(table_np=t) for t in (1, 2, 4, 8)] + \
     [dict(horner_form=h, groups_form=g) for h, g in ((1, 1), (2, 2), (3, 3), (3, 1), (2, 3))] + \
     [dict(fixed_chunk_gens=c) for c in (-1, 3)]
STRAUS = [dict(verify_window_parallel=0, verify_straus_np=n) for n in (1, 2, 3, 4)] + \
         [dict(verify_window_parallel=0, verify_no_fuse=1, verify_straus_np=n) for n in (1, 4)]


def _id(route):
    return "-".join("%s=%d" % (k.replace("verify_", ""), v) for k, v in route.items())


@pytest.mark.parametrize("route", WP + STRAUS, ids=_id)
def test_verify_batch_routes(gpu, opts, batch, route):
    """70 proofs through the window-parallel launches -- every table lane shape, every form of the two Horner stages, the generator
    half in both of its lane shapes -- and through the Straus launches with 1..4 points per lane, fused and separate"""
    opts(**route)
    check_batch(gpu, batch, pick(batch, 70))


def test_verify_batch_latency_mode(gpu, batch):
    gpu.set_latency_mode(True)
    try:
        check_batch(gpu, batch, pick(batch, 70))
    finally:
        gpu.set_latency_mode(False)


@pytest.mark.parametrize("tnp", [1, 8])
@pytest.mark.parametrize("nb", [1, 5])
def test_verify_handful(gpu, opts, batch, nb, tnp):
    """a single `line` proof, and five proofs of five kinds (one honest), through the launches a handful of proofs takes"""
    opts(table_np=tnp)
    recs = pick(batch, nb)
    assert recs[0].kind == "line" and len({r.kind for r in recs}) == nb
    check_batch(gpu, batch, recs)


def test_verify_with_device_transcript(gpu, batch):
    """the challenges the device derives over the crafted points are the oracle's, and so are the verdicts and mega_check points"""
    import pymodel as pm
    recs = pick(batch, 70)
    nb = len(recs)
    ok, mega, ch = gpu.r1cs_verify_batch_fs(batch.g, batch.circ, nb, batch.n1, batch.k, batch.m, pm.Transcript(dc.LABEL).state * nb,
                                            cat(recs, "points"), cat(recs, "scalars"))
    assert ch == cat(recs, "challenges")
    assert ok == [r.ok for r in recs]
    assert mega == cat(recs, "mega")


def weighted_sum(recs, rhos):
    acc = dc.IDENT
    for r, w in zip(recs, rhos):
        acc = o.point_add(acc, o.point_mul(w, r.mega))
    return acc


def rhos(seed, n):
    rnd = random.Random(seed)
    return [o.s2b(rnd.randrange(1, o.N)) for _ in range(n)]


@pytest.mark.parametrize("nb", [70, 14])
def test_combined_check_and_screening(gpu, opts, batch, nb):
    """sum_p rho_p * mega_check_p over the crafted batch: 70 proofs take the one-instance bucket pipeline (pippenger2_supported:
    from 256 terms on, 18 per proof), 14 proofs the generic launches; then the screened call, whose verdicts are the oracle's"""
    assert 70 * NVAR >= 256 > 14 * NVAR
    recs = pick(batch, nb)
    rho = rhos(nb, nb)
    args = (batch.g, batch.circ, nb, batch.n1, batch.k)
    got = gpu.r1cs_verify_combined(*args, batch.m, cat(recs, "points"), cat(recs, "scalars"), cat(recs, "challenges"), b"".join(rho))
    assert got == weighted_sum(recs, rho)
    assert got != dc.IDENT
    opts(stream_batch=16, screen_batch=16, stream_lanes=3)
    ok, nf = gpu.r1cs_verify_screened(*args, cat(recs, "points"), cat(recs, "scalars"), cat(recs, "challenges"), b"".join(rho))
    assert ok == [r.ok for r in recs]
    assert nf >= 1


@pytest.fixture(scope="module")
def mixed(gpu, batch):
    """two groups for the ragged calls: 12 of the 8-bit proofs, and 8 proofs of the 32-bit range gadget crafted in the same ways"""
    recs32 = [dc.make_rec(kind, 700 + i, 32, 8, tamper) for i, (kind, tamper) in enumerate(
        [(None, False), ("twin", False), ("line", False), (None, True), ("opposite", False), ("gens", False), ("line_B", False), (None, False)])]
    r0 = recs32[0]
    assert r0.k == 5 and all(r.ok == (1 if r.kind == "honest" else 0) for r in recs32 if r.kind in ("honest", "tampered"))
    circ = gpu.circuit_create(*r0.csr, r0.n, r0.m)
    g = gpu.gens_create(o.gens("G", 32), o.gens("H", 32), o.generator(), o.generator(), 8)
    yield SimpleNamespace(g=g, sets=[(batch.circ, pick(batch, 12)), (circ, recs32)])
    gpu.gens_destroy(g)
    gpu.circuit_destroy(circ)


def _groups(mixed, seed, honest_only=False):
    groups, all_recs, all_rho = [], [], []
    for i, (circ, recs) in enumerate(mixed.sets):
        recs = [r for r in recs if r.kind == "honest"] if honest_only else recs
        rho = rhos(seed + i, len(recs))
        groups.append(dict(circuit=circ, nb=len(recs), n1=recs[0].n1, k=recs[0].k, points=cat(recs, "points"), scalars=cat(recs, "scalars"),
                           challenges=cat(recs, "challenges"), gadget_challenges=None, rho=b"".join(rho)))
        all_recs += recs
        all_rho += rho
    return groups, all_recs, all_rho


def test_mixed_combined_and_screened(gpu, mixed):
    """bpgpu_r1cs_verify_mixed_combined / _screened over two circuits with crafted proofs in both groups"""
    groups, recs, rho = _groups(mixed, 31)
    got = gpu.r1cs_verify_mixed_combined(mixed.g, groups)
    assert got == weighted_sum(recs, rho) != dc.IDENT
    oks, nf = gpu.r1cs_verify_mixed_screened(mixed.g, groups)
    assert [b for ok in oks for b in ok] == [r.ok for r in recs]
    assert nf >= 1
    groups, recs, rho = _groups(mixed, 32, honest_only=True)
    assert len(recs) >= 3 and gpu.r1cs_verify_mixed_combined(mixed.g, groups) == dc.IDENT


@pytest.fixture(scope="module")
def gens32(gpu):
    g = gpu.gens_create(o.gens("G", 32), o.gens("H", 32), o.generator(), o.generator(), 8)
    yield g
    gpu.gens_destroy(g)


@pytest.mark.parametrize("nb", [3, 70])
@pytest.mark.parametrize("n", [4, 32])
def test_inner_product_verification(gpu, gens32, n, nb):
    """InnerProductProof::verify with R_j = +-L_j and with all L_j, R_j on one line: the expect_P of these operands is accepted as
    P and returned byte for byte, P + B is rejected, and so is P := L_0 (the oracle's verdicts), over caller-supplied and over
    resident generators"""
    recs = dc.ipp_batch(n, nb)
    want, want_shifted = [r["bit"] for r in recs], [r["bit_shifted"] for r in recs]
    assert want[1] == 0 and want.count(1) == nb - 1 and want_shifted == [0] * nb

    def j(key):
        return b"".join(r[key] for r in recs)
    tail = (j("L"), j("R"), j("ab"), j("ch"))
    ok, expect = gpu.ipp_verify_batch(nb, n, j("Q"), j("Gf"), j("Hf"), recs[0]["G"], recs[0]["H"], True, j("P"), *tail, want_expect=True)
    assert ok == want and expect == j("expect")
    assert gpu.ipp_verify_batch(nb, n, j("Q"), j("Gf"), j("Hf"), recs[0]["G"], recs[0]["H"], True, j("P_shifted"), *tail) == want_shifted
    ok, expect = gpu.ipp_verify_gens(gens32, nb, n, j("w"), j("Gf"), j("Hf"), j("P"), *tail, want_expect=True)
    assert ok == want and expect == j("expect")
    assert gpu.ipp_verify_gens(gens32, nb, n, j("w"), j("Gf"), j("Hf"), j("P_shifted"), *tail) == want_shifted
