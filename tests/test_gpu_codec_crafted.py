"""The point codec on the encodings of tests/codec_cases.py: x whose square root has chosen discrete-logarithm digits (zero digits,
runs of 0xFF, the carry of the halved exponent, odd order, non-residues), y next to the sign boundary, x next to and past p.
Every expectation is the Python model's (oracle/pymodel.py point_decompress / point_compress: plain Tonelli-Shanks), every
comparison byte equality.  Run with `-m gpu` on an MI355X."""
import pytest

import bp_helpers as bh
import codec_cases as cc
import oracle_lib as o
from codec_cases import P, pm

pytestmark = pytest.mark.gpu
KINDS = ("valid", "nonresidue", "noncanonical", "identity")


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def want():
    """encoding -> (ok, 64 bytes) of the model, computed once"""
    return {c.enc: cc.model_decode(c.enc) for c in cc.build().cases}


def _check(gpu, want, cases, tag):
    got, ok = gpu.points_decompress(b"".join(c.enc for c in cases))
    for i, c in enumerate(cases):
        w_ok, w_xy = want[c.enc]
        assert ok[i] == w_ok, (tag, i, c.name, ok[i])
        assert got[64 * i:64 * i + 64] == w_xy, (tag, i, c.name)


def test_first_use_of_a_context_decodes_the_single_digit_family(want):
    """the square-root tables are built on the stream of the call that first needs them: here that call is the crafted one"""
    import mpc_bulletproof_amd as m
    cases = [c for c in cc.build().cases if c.name.startswith(cc.SINGLE_DIGIT)]
    assert len(cases) == 6 * 4 * 3
    fresh = m.BpGpu(0)
    try:
        _check(fresh, want, cases, "fresh")
    finally:
        fresh.close()


def test_all_crafted_encodings_in_one_call(gpu, want):
    cases = list(cc.build().cases)
    assert len(cases) > 200 and {c.kind for c in cases} == set(KINDS)
    _check(gpu, want, cases, "all")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_lane_mixes(gpu, want, n):
    """launches of one lane, a wave less one, a wave, a wave and one, two waves and one: valid, non-residue, non-canonical and
    identity encodings alternate lane by lane, and the last lane of the last block (the one the dead lanes are clamped to) is each
    kind in turn"""
    pools = {k: [c for c in cc.build().cases if c.kind == k] for k in KINDS}
    for last in range(4):
        shift = (last - (n - 1)) % 4
        cases = []
        for i in range(n):
            pool = pools[KINDS[(i + shift) % 4]]
            cases.append(pool[(i // 4 + 7 * last) % len(pool)])
        assert cases[-1].kind == KINDS[last] and (n < 4 or {c.kind for c in cases[:4]} == set(KINDS))
        _check(gpu, want, cases, (n, KINDS[last]))


def test_compress_gives_back_the_canonical_encoding(gpu, want):
    import mpc_bulletproof_amd as m
    b = cc.build()
    valid = [c for c in b.cases if c.kind == "valid"]
    xy = b"".join(want[c.enc][1] for c in valid)
    assert gpu.points_compress(xy) == b"".join(c.enc for c in valid)
    # the points next to the sign boundary and at the ends of the x range, by their coordinates; the identity among them
    pts = list(b.sign_points) + list(b.x_points) + [(x, P - y) for x, y in b.sign_points]
    enc = gpu.points_compress(b"".join(pm.p2b(pt) for pt in pts) + bytes(64))
    assert enc == b"".join(pm.point_compress(pt) for pt in pts) + bytes(31) + b"\x40"
    half = (P - 1) // 2
    for i, (x, y) in enumerate(pts):
        assert enc[32 * i + 31] >> 6 == (2 if y > half else 0), (hex(x), hex(y))
    assert {y for _, y in pts} >= {half - 1, half + 2, 2, P - 2}
    # y >= p, and y off by one, are refused
    good = pm.p2b(b.sign_points[0]) * 3
    for x, y in list(b.sign_points) + list(b.x_points[:2]):
        for bad_y in (y + P, y + 1, y - 1):
            bad = x.to_bytes(32, "little") + bad_y.to_bytes(32, "little")
            for data in (bad, good + bad, bad + good):
                with pytest.raises(m.BpGpuError) as e:
                    gpu.points_compress(data)
                assert e.value.code == m.lib.E_ARG, (hex(x), hex(bad_y))


def test_wire_scalars_lifted_by_the_largest_multiple_of_n(gpu):
    """bpgpu_r1cs_verify_batch_wire reads the five big-endian scalars modulo n: a proof whose scalars are each lifted by the largest
    multiple of n that stays below 2^256 (up to 31 n) is the same proof; one whose b is lifted by that multiple plus one has b + 1"""
    nb, n_bits = 8, 8
    recs, cap = bh.make_range_batch(n_bits, nb)
    s0 = o.VerifySession(o.K_RANGE, n_bits, b"RangeProofTest", [], recs[0][1], recs[0][0], cap)
    rp, kind, idx, coeff = s0.csr()
    circ = gpu.circuit_create(rp, kind, idx, coeff, s0.n1 + s0.n2, s0.m)
    gens = gpu.gens_create(o.gens("G", cap), o.gens("H", cap), o.generator(), o.generator(), 8)
    try:
        names = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6")
        wires = []
        for proof, _ in recs:
            k, pts11, sc3, L, R, ab = bh.parse_flat_proof(proof)
            p = {nm: pm.b2p(pts11[64 * i:64 * i + 64]) for i, nm in enumerate(names)}
            p.update({nm: pm.b2s(sc3[32 * i:32 * i + 32]) for i, nm in enumerate(("t_x", "t_x_blinding", "e_blinding"))})
            p["L_vec"] = [pm.b2p(L[64 * i:64 * i + 64]) for i in range(k)]
            p["R_vec"] = [pm.b2p(R[64 * i:64 * i + 64]) for i in range(k)]
            p["a"], p["b"] = pm.b2s(ab[:32]), pm.b2s(ab[32:])
            wires.append(pm.r1cs_proof_to_bytes(p))
        coms = [pm.point_compress(pm.b2p(com)) for _, com in recs]
        plen = len(wires[0])
        k = s0.k
        assert plen == 1 + (8 + 3 + 2 * k + 2) * 32
        offs = [1 + 32 * (8 + q) for q in range(3)] + [1 + 32 * (8 + 3 + 2 * k + q) for q in range(2)]

        def lifted(wire, which, extra=0):
            w = bytearray(wire)
            for off in which:
                v = int.from_bytes(w[off:off + 32], "big")
                assert v < pm.N
                top = ((1 << 256) - 1 - v - extra) // pm.N
                assert 29 <= top <= 31 and v + top * pm.N + extra < 1 << 256 <= v + (top + 1) * pm.N + extra
                w[off:off + 32] = (v + top * pm.N + extra).to_bytes(32, "big")
            return bytes(w)
        wires[2] = lifted(wires[2], offs)
        wires[5] = lifted(wires[5], offs[4:], extra=1)
        # the oracle on the reduced values: proof 2 unchanged, proof 5 with b + 1
        flat5 = recs[5][0][:-32] + pm.s2b((pm.b2s(recs[5][0][-32:]) + 1) % pm.N)
        flats = [r[0] for r in recs]
        flats[5] = flat5
        sessions = [o.VerifySession(o.K_RANGE, n_bits, b"RangeProofTest", [], com, flat, cap) for flat, (_, com) in zip(flats, recs)]
        expect = [1 if s.rc == 0 else 0 for s in sessions]
        for s in sessions:
            s.close()
        assert expect == [1, 1, 1, 1, 1, 0, 1, 1]
        init = pm.Transcript(b"RangeProofTest").state * nb
        assert gpu.r1cs_verify_batch_wire(gens, circ, nb, s0.n1, plen, b"".join(wires), b"".join(coms), init) == expect
    finally:
        s0.close()
        gpu.gens_destroy(gens)
        gpu.circuit_destroy(circ)
