"""mul2 of csrc/fe29.cuh, (a b + c d) / R with ONE Montgomery reduction, on the DEVICE (the asm MAD chains, which the CPU build of
tests/test_fused_products_cpu.py does not run; tests/csrc/mul2_gpu_test.hip, built by __graft_entry__.build()), the point additions
of csrc/ec29.cuh that take their Y through it, and the verifier end to end on its smallest shapes.  Operands and expected values:
tests/fused_product_cases.py (Python big integers, the Python model) and the CPU oracle; nothing is compared with another GPU
result.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import os
from types import SimpleNamespace

import pytest

import bp_helpers as bh
import fused_product_cases as fc
import oracle_lib as o
import window_digits as wd

pm = fc.pm
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LABEL = b"RangeProofTest"


@pytest.fixture(scope="module")
def g():
    so = os.path.join(HERE, "csrc", "libmul2_gpu.so")
    assert os.path.exists(so), "tests/csrc/libmul2_gpu.so missing: run __graft_entry__.build()"
    return C.CDLL(so)


def _ints(b, n):
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(n)]


def test_mul2_on_raw_limbs_at_the_contract_bounds_on_device(g):
    """the cases of the CPU test -- every limb at +-(2^29 + 8), every column at its maximum of either sign, the two products at
    opposite maxima, results 0 and +-1, canonical, raw and difference-shaped operands -- in ONE launch of 256 lanes"""
    cases = fc.mul2_cases()
    n = len(cases)
    assert 200 <= n <= 512
    flat = [x for _, case in cases for v in case for x in v]
    out = (C.c_uint8 * (32 * n))()
    assert g.m2g_mul2((C.c_int32 * len(flat))(*flat), C.c_size_t(n), out, None) == 0, "no HIP device"
    for (name, case), got in zip(cases, _ints(bytes(out), n)):
        assert got == fc.want(case), name


def test_mul2_with_a_zero_second_product_equals_mul_on_device(g):
    cases = fc.mul_edge_cases()
    n = len(cases)
    flat = [x for a, b, d in cases for v in (a, b, [0] * 9, d) for x in v]
    out, out2 = (C.c_uint8 * (32 * n))(), (C.c_uint8 * (32 * n))()
    assert g.m2g_mul2((C.c_int32 * len(flat))(*flat), C.c_size_t(n), out, out2) == 0, "no HIP device"
    for (a, b, d), fused, plain in zip(cases, _ints(bytes(out), n), _ints(bytes(out2), n)):
        assert fused == plain == fc.value(a) * fc.value(b) * fc.RINV % fc.P, (a, b)


def test_changed_additions_on_16_x_16_point_pairs_on_device(g):
    """(identity, G, -G, 2G, 12 random points), all pairs: P + P, P + (-P) and the identity on either side take the out-of-line
    exact cases (which keep the two-product Y), every other pair the inlined addition with the fused Y"""
    pts = fc.points(12)
    pairs = [(a, b) for a in pts for b in pts]
    n = len(pairs)
    assert n == 256
    a = (C.c_uint8 * (64 * n)).from_buffer_copy(b"".join(pm.p2b(x) for x, _ in pairs))
    b = (C.c_uint8 * (64 * n)).from_buffer_copy(b"".join(pm.p2b(y) for _, y in pairs))
    out, rc = (C.c_uint8 * (64 * n))(), (C.c_int * n)()
    for op in fc.POINT_OPS:
        assert g.m2g_point(op, a, b, C.c_size_t(n), out, rc) == 0, "no HIP device"
        ob = bytes(out)
        for i, (x, y) in enumerate(pairs):
            if op in (4, 5) and y is pm.INF:
                assert rc[i] == -3
                continue
            assert rc[i] == 0 and pm.b2p(ob[64 * i:64 * i + 64]) == pm.pt_add(x, y), (op, i, x, y)


# ------------------------------------------------------------------ the verifier end to end
@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    ctx = m.BpGpu(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def proofs(gpu):
    """four proofs of the 8-bit range gadget from the oracle, the third tampered; larger batches repeat them in turn"""
    recs, cap = bh.make_range_batch(8, 4, seed0=8800, tamper={2})
    out, dims = [], None
    for proof, com in recs:
        s = o.VerifySession(o.K_RANGE, 8, LABEL, [], com, proof, cap)
        k, pts, sc = bh.verify_inputs(proof, com)
        out.append(SimpleNamespace(points=pts, scalars=sc, challenges=s.challenges(), terms_sc=s.msm_terms()[0], mega=s.mega_check(), rc=s.rc))
        dims = SimpleNamespace(n1=s.n1, k=s.k, m=s.m, n=s.n1 + s.n2, csr=s.csr())
        s.close()
    assert [r.rc == 0 for r in out] == [True, True, False, True]
    circ = gpu.circuit_create(*dims.csr, dims.n, dims.m)
    yield SimpleNamespace(recs=out, cap=cap, circ=circ, n1=dims.n1, k=dims.k, m=dims.m)
    gpu.circuit_destroy(circ)


@pytest.mark.parametrize("c", [8, 16])
@pytest.mark.parametrize("nb,chunk_gens", [(3, -1), (257, 3)])
def test_verifier_end_to_end_on_smallest_shapes(gpu, proofs, nb, chunk_gens, c):
    """8-bit range proofs over a c-bit generator table: nb = 3 with the generator half on lanes per proof (fixed_chunk_gens = -1),
    nb = 257 with a proof per lane in runs of 3 generators (k_verify_back_q: fixed_chunk_body); a valid and a tampered proof in
    each.  At c = 16 the generator half rides in the back launch; at c = 8 the gadget's 18 x 32 (generator, window) pairs are more
    than one chunk and it is k_fixed_msm's launch: the same addition.  The window sums (k_verify_windows), the Horner stages and
    the verdict's partial sums run in all four.  Accept bits, mega_check and every MSM scalar against the oracle's; the signed
    recoding of those scalars saw digits of both signs at the table's width and at the window sums' 4 bits, and zero digits at 4 and 8."""
    recs = [proofs.recs[i % 4] for i in range(nb)]
    for width in (c, 4):
        ds = [d for r in recs[:4] for s in o.unscalars(r.terms_sc) for d in wd.digits(s, width)]
        assert min(ds) < 0 < max(ds)
        assert width > 8 or 0 in ds          # (a random 16-bit window is zero once in 65 536: not among these 2 304)
    old = gpu.get_option("fixed_chunk_gens")
    gens = gpu.gens_create(o.gens("G", proofs.cap), o.gens("H", proofs.cap), o.generator(), o.generator(), c)
    try:
        gpu.set_option("fixed_chunk_gens", chunk_gens)
        cat = lambda key: b"".join(getattr(r, key) for r in recs)      # noqa: E731
        ok, mega, full = gpu.r1cs_verify_batch(gens, proofs.circ, nb, proofs.n1, proofs.k, proofs.m, cat("points"), cat("scalars"),
                                               cat("challenges"), True, True)
        assert ok == [1 if r.rc == 0 else 0 for r in recs] and 0 in ok and 1 in ok
        assert mega == cat("mega")
        assert full == cat("terms_sc")
    finally:
        gpu.set_option("fixed_chunk_gens", old)
        gpu.gens_destroy(gens)
