"""bpgpu_r1cs_commit_values / _dev and bpgpu_mpc_commit_values -- Prover::commit for every committed value, transcript included --
against the Python model (oracle/pymodel.py through tests/commit_cases.py): bytes on every launch route of the point path and both
blocks of the chain launch, edge pairs over equal bases, the chain commit -> constraints_satisfied -> prove_fs without a host wait
and on to the wire verifiers, malformed input, and the two-party form under the test dealer.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import itertools

import pytest

import circuit_gen as cg
import commit_cases as cc
import mpc_dealer as md
import oracle_lib as o
import prove_fs2_cases as pc2
import prove_fs_cases as pc

pm = cg.pm
N = pm.N
pytestmark = pytest.mark.gpu
CAP = 64
cut = md.cut


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


BASES = {"equal": (cc.base_G, cc.base_G), "distinct": (cc.base_G, cc.base_H0)}
_gens = {}


@pytest.fixture(scope="module")
def gens_for(gpu):
    """generator handles by (bases, window bits): capacity 2, made once"""
    def get(bases, c=8):
        if (bases, c) not in _gens:
            B, Bb = (f() for f in BASES[bases])
            _gens[(bases, c)] = gpu.gens_create(o.gens("G", 2), o.gens("H", 2), pm.p2b(B), pm.p2b(Bb), c)
        return _gens[(bases, c)]
    yield get
    for h in _gens.values():
        gpu.gens_destroy(h)
    _gens.clear()


@pytest.fixture(scope="module")
def gens(gpu):
    """the provers' generators: B = B_blinding = the curve generator, as the model's PedersenGens"""
    g = gpu.gens_create(o.gens("G", CAP), o.gens("H", CAP), o.generator(), o.generator(), 8)
    yield g
    gpu.gens_destroy(g)


_expect = {}


def case(bases, nb, m):
    """values, operands and the model's expectation of a shape over a pair of bases (computed once, left unchanged)"""
    if (bases, nb, m) not in _expect:
        v, vb = cc.values(1000 * nb + m, nb, m)
        init = cc.init_states(nb)
        B, Bb = (f() for f in BASES[bases])
        _expect[(bases, nb, m)] = (cc.ark(v), cc.ark(vb), b"".join(init), cc.expect(v, vb, B, Bb, init))
    return _expect[(bases, nb, m)]


def run_dev(gpu, g, nb, m, v, vb, init, want=(True, True, True)):
    """the `_dev` form on fresh device buffers -> (V, V_compressed, states_out, input flag), None for an output not asked for"""
    sizes = (64 * nb * m, 32 * nb * m, 32 * nb)
    ins = [gpu.to_device(x) if x else None for x in (v, vb)]
    d_init = gpu.to_device(init) if want[2] else None
    outs = [gpu.malloc(max(s, 32)) if w else None for s, w in zip(sizes, want)]
    try:
        gpu.r1cs_commit_values_dev(g, nb, m, ins[0], ins[1], d_init, *outs)
        flag = gpu.input_flag()
        return tuple(gpu.download(p, s) if p is not None else None for p, s in zip(outs, sizes)) + (flag,)
    finally:
        for p in ins + [d_init] + outs:
            if p is not None:
                gpu.free(p)


# ------------------------------------------------------------------------------------------------ 1: the model's bytes
@pytest.mark.parametrize("bases", sorted(BASES))
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "nb%d-m%d" % s)
def test_bytes_equal_the_model_in_both_forms(gpu, gens_for, shape, bases):
    """V, V_compressed and states_out together, host form and `_dev` form, at c = 8"""
    nb, m = shape
    v, vb, init, e = case(bases, nb, m)
    g = gens_for(bases)
    V, Vc, so = gpu.r1cs_commit_values(g, nb, m, v or None, vb or None, init)
    assert V == e["V"], "V"
    assert Vc == e["V_compressed"], "V_compressed"
    assert so == e["states_out"], "states_out"
    assert run_dev(gpu, g, nb, m, v, vb, init) == (V, Vc, so, 0)


@pytest.mark.parametrize("bases", sorted(BASES))
@pytest.mark.parametrize("c", (4, 16))
def test_other_table_widths(gpu, gens_for, c, bases):
    nb, m = 5, 13
    v, vb, init, e = case(bases, nb, m)
    assert gpu.r1cs_commit_values(gens_for(bases, c), nb, m, v, vb, init) == (e["V"], e["V_compressed"], e["states_out"])


@pytest.mark.parametrize("shape", ((3, 2), (5, 13)), ids=lambda s: "nb%d-m%d" % s)
def test_every_subset_of_the_outputs_gives_the_same_bytes(gpu, gens_for, shape):
    nb, m = shape
    v, vb, init, e = case("equal", nb, m)
    g = gens_for("equal")
    full = (e["V"], e["V_compressed"], e["states_out"])
    for want in itertools.product((False, True), repeat=3):
        if not any(want):
            continue
        host = gpu.r1cs_commit_values(g, nb, m, v, vb, init if want[2] else None, want_points=want[0], want_compressed=want[1])
        assert host == tuple(x if w else None for x, w in zip(full, want)), want
        assert run_dev(gpu, g, nb, m, v, vb, init, want) == host + (0,), want


# ------------------------------------------------------------------------------------------------ 2: edge pairs over equal bases
@pytest.mark.parametrize("shape", cc.EDGE_SHAPES, ids=lambda s: "%d-commitments" % (s[0] * s[1]))
def test_edge_pairs_over_equal_bases(gpu, gens_for, shape):
    """sums that vanish, sums that are doublings, and scalars whose every window digit is an extreme of the recoding, in each of the
    three point routes: the two terms of a commitment read the same table, so partial sums coincide inside the block and butterfly sums"""
    nb, m = shape
    g = gens_for("equal")
    init = cc.init_states(nb)
    for v, vb in cc.edge_batches(8, nb, m):
        e = cc.expect(v, vb, pm.G, pm.G, init)
        V, Vc, so = gpu.r1cs_commit_values(g, nb, m, cc.ark(v), cc.ark(vb), b"".join(init))
        flat = [(a, b) for rv, rb in zip(v, vb) for a, b in zip(rv, rb)]
        for i, (a, b) in enumerate(flat):
            assert V[64 * i:64 * i + 64] == e["V"][64 * i:64 * i + 64], ("V", i, hex(a), hex(b))
            assert Vc[32 * i:32 * i + 32] == e["V_compressed"][32 * i:32 * i + 32], ("V_compressed", i, hex(a), hex(b))
            if (a, b) in cc.IDENTITY_PAIRS:
                assert V[64 * i:64 * i + 64] == bytes(64) and Vc[32 * i:32 * i + 32] == bytes(31) + b"\x40", i
        assert so == e["states_out"]


# ------------------------------------------------------------------------------------------------ 3: the chain of calls
@pytest.mark.parametrize("shape", cc.CHAIN_SHAPES, ids=lambda s: "n%d-m%d-q%d-nb%d" % s[:4])
def test_commit_check_and_prove_without_a_host_wait(gpu, gens, shape):
    """commit_values_dev -> constraints_satisfied_dev -> prove_fs_dev on one stream, v and v_blinding shared: the proofs' wire bytes
    are the model's, the wire verifier accepts them from the commit call's own inputs and outputs, and a commitment to another value
    is rejected -- that proof alone"""
    n, m, q, nb, _ = shape
    circ, recs = cc.chain_case(shape)
    kw = pc.operands(recs, False)
    k = pc.lg_padded(n)
    plen = 1 + 11 * 32 + (2 * k + 2) * 32
    init = b"".join(pm.Transcript(pc.label(p)).state for p in range(nb))
    v = cc.ark([circ.v] * nb)
    h = gpu.circuit_create(*circ.csr(), circ.n, circ.m)
    bufs = []

    def dev(data):
        bufs.append(gpu.to_device(data) if data else None)
        return bufs[-1]

    def room(nbytes):
        bufs.append(gpu.malloc(max(nbytes, 32)))
        return bufs[-1]
    try:
        d_v, d_vb, d_init = dev(v), dev(kw["v_blinding"] or b""), dev(init)
        d_aL, d_aR, d_aO, d_sL, d_sR, d_bl = (dev(kw[x]) for x in ("a_L", "a_R", "a_O", "s_L", "s_R", "blindings"))
        d_V, d_Vc, d_st, d_ok = room(64 * nb * m), room(32 * nb * m), room(32 * nb), room(4 * nb)
        d_pts, d_sc, d_wire = room(64 * nb * (11 + 2 * k)), room(160 * nb), room(nb * plen)
        gpu.r1cs_commit_values_dev(gens, nb, m, d_v, d_vb, d_init, d_V, d_Vc, d_st)
        gpu.r1cs_constraints_satisfied_dev(h, nb, d_aL, d_aR, d_aO, d_ok, d_v=d_v)
        gpu.r1cs_prove_fs_dev(gens, h, nb, d_st, d_aL, d_aR, d_aO, d_bl, d_pts, d_sc, d_v_blinding=d_vb, d_s_L=d_sL, d_s_R=d_sR, d_wire=d_wire)
        assert gpu.input_flag() == 0                                      # the first wait; the flag is prove_fs_dev's (every _dev call resets it):
        # what the commit call wrote is checked by its bytes below
        wire, Vc, st = gpu.download(d_wire, nb * plen), gpu.download(d_Vc, 32 * nb * m), gpu.download(d_st, 32 * nb)
        assert gpu.download(d_ok, 4 * nb) == (1).to_bytes(4, "little") * nb
        assert st == kw["states"]
        assert Vc == b"".join(pm.point_compress(pt) for r in recs for pt in r["V"])
        assert gpu.download(d_V, 64 * nb * m) == b"".join(pm.p2b(pt) for r in recs for pt in r["V"])
        assert wire == b"".join(r["wire"] for r in recs)
        assert gpu.r1cs_verify_batch_wire(gens, h, nb, n, plen, wire, Vc, init) == [1] * nb
        if m:
            # prover 1 commits to v_0 + 1 instead: one changed commitment
            other = [list(circ.v) for _ in range(nb)]
            other[1][0] = (other[1][0] + 1) % N
            Vc2 = gpu.r1cs_commit_values(gens, nb, m, cc.ark(other), kw["v_blinding"], want_points=False)[1]
            assert [a != b for a, b in zip(cut(Vc, 32), cut(Vc2, 32))] == [i == m for i in range(nb * m)]
            assert gpu.r1cs_verify_batch_wire(gens, h, nb, n, plen, wire, Vc2, init) == [1, 0] + [1] * (nb - 2)
    finally:
        for b in bufs:
            if b is not None:
                gpu.free(b)
        gpu.circuit_destroy(h)


def test_commit_then_prove_in_two_phases(gpu, gens):
    """commit_values -> prove_fs2_begin / _finish -> verify_batch_wire2 on a generated two-phase circuit"""
    nb, vkeys = cc.CHAIN2_NB, (False, False)
    circ, recs = cc.chain2_case()
    m, k = circ.m, pc.lg_padded(circ.n)
    plen = 1 + 14 * 32 + (2 * k + 2) * 32
    init = b"".join(pm.Transcript(pc.label(p)).state for p in range(nb))
    vb = b"".join(r["v_blinding"] for r in recs)
    h = gpu.circuit_create_param(circ.q, 1, *circ.csr_param(), circ.n, circ.m)
    try:
        V, Vc, st = gpu.r1cs_commit_values(gens, nb, m, cc.ark([circ.v] * nb), vb, init)
        assert st == b"".join(r["state_in"] for r in recs)
        assert V == b"".join(pm.p2b(pt) for r in recs for pt in r["V"])
        sess = gpu.r1cs_prove_fs2_begin(gens, h, nb, circ.n1, gadget_label=cg.CHI_LABEL, **dict(pc2.begin_operands(recs, vkeys, circ.n1), states=st))[0]
        wire = gpu.r1cs_prove_fs2_finish(gens, h, sess, nb, circ.n, m, **pc2.finish_operands(recs, vkeys))[2]
        assert wire == b"".join(r["wire"] for r in recs)
        assert gpu.r1cs_verify_batch_wire2(gens, h, nb, circ.n1, plen, cg.CHI_LABEL, wire, Vc, init) == [1] * nb
    finally:
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ 4: malformed input, the empty batch
def test_a_non_canonical_limb_and_the_empty_batch(gpu, gens_for):
    import mpc_bulletproof_amd as mm
    nb, m = 3, 2
    v, vb, init, e = case("equal", nb, m)
    g = gens_for("equal")
    full = (e["V"], e["V_compressed"], e["states_out"])
    order = N.to_bytes(32, "little")                                      # the group order itself: not below the modulus
    for bad_v, bad_vb in ((v[:96] + order + v[128:], vb), (v, order + vb[32:])):
        with pytest.raises(mm.lib.BpGpuError) as err:
            gpu.r1cs_commit_values(g, nb, m, bad_v, bad_vb, init)
        assert err.value.code == mm.lib.E_ARG
        assert run_dev(gpu, g, nb, m, bad_v, bad_vb, init)[3] == 1
        assert gpu.input_flag() == 0                                      # reading cleared it
        assert run_dev(gpu, g, nb, m, v, vb, init) == full + (0,)         # the context is usable afterwards
        assert gpu.r1cs_commit_values(g, nb, m, v, vb, init) == full
    with pytest.raises(mm.lib.BpGpuError) as err:
        gpu.mpc_commit_values(g, 1, 2, order * 6, bytes(32 * 6))
    assert err.value.code == mm.lib.E_ARG
    # nb == 0: BPGPU_OK, nothing written
    outs = [(C.c_uint8 * 64)(*([0x5A] * 64)) for _ in range(3)]
    assert mm.lib._lib.bpgpu_r1cs_commit_values(gpu.ctx, g, 0, m, None, None, init, *outs) == 0
    d = gpu.to_device(b"\x5A" * 64)
    try:
        assert mm.lib._lib.bpgpu_r1cs_commit_values_dev(gpu.ctx, g, 0, m, None, None, d, d, d, d) == 0
        assert gpu.download(d, 64) == b"\x5A" * 64
    finally:
        gpu.free(d)
    assert all(bytes(x) == b"\x5A" * 64 for x in outs)


# ------------------------------------------------------------------------------------------------ 5: two parties
@pytest.fixture(scope="module")
def parties(gpu):
    import mpc_bulletproof_amd as m
    g1 = m.BpGpu(0)
    gs = [gpu, g1]
    hs = [x.gens_create(o.gens("G", 2), o.gens("H", 2), pm.p2b(cc.base_G()), pm.p2b(cc.base_H0()), 8) for x in gs]
    yield gs, hs
    for x, h in zip(gs, hs):
        x.gens_destroy(h)
    g1.close()


def two_party(parties, nb, m, tamper=False):
    """-> (the opened commitments' bytes, the model's, the dealer)"""
    gs, hs = parties
    dealer = md.Dealer(77 + nb)
    v, vb = cc.values(5000 + 10 * nb + m, nb, m)
    sv, sb = [dealer.share_vec(row) for row in v], [dealer.share_vec(row) for row in vb]      # [prover][party][plane][j]
    if tamper:
        sv[0][0][1][0] = (sv[0][0][1][0] + 1) % N                        # party 0's MAC share of v[0][0]
    outs = []
    for q in range(2):
        planes = lambda sh: md.pack([[sh[p][q][k] for k in range(3)] for p in range(nb)])      # noqa: E731
        outs.append(gs[q].mpc_commit_values(hs[q], nb, m, planes(sv), planes(sb)))
    opened = b""
    for p in range(nb):
        for j in range(m):
            planes = [[outs[q][((p * 3 + k) * m + j) * 64:((p * 3 + k) * m + j + 1) * 64] for k in range(3)] for q in range(2)]
            opened += dealer.open_pt("V[%d][%d]" % (p, j), planes)
    want = b"".join(pm.p2b(cc.commit(a, b, cc.base_G(), cc.base_H0())) for rv, rb in zip(v, vb) for a, b in zip(rv, rb))
    return opened, want, dealer


@pytest.mark.parametrize("shape", ((1, 1), (2, 5), (22, 3)), ids=lambda s: "nb%d-m%d" % s)
def test_two_parties_open_the_models_commitments(parties, shape):
    opened, want, dealer = two_party(parties, *shape)
    assert opened == want
    assert dealer.bad == [] and dealer.mod_mismatch == []


def test_a_tampered_mac_share_is_reported_under_its_name(parties):
    opened, want, dealer = two_party(parties, 2, 5, tamper=True)
    assert opened == want                                                 # the share planes are untouched
    assert dealer.bad == ["V[0][0]"] and dealer.mod_mismatch == []
