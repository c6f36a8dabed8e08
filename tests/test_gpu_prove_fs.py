"""bpgpu_r1cs_prove_fs / _dev -- Prover::prove in one device call, transcript included -- against the Python model
(oracle/pymodel.py: Prover.prove under a replay RNG, tests/prove_fs_cases.py) on generated circuits, against the staged entry points,
against the verifiers, and through the host mirror (BPH_PROVE_FUSED).  Run with `-m gpu` on an MI355X."""
import ctypes as C
import os
import random

import pytest

import circuit_gen as cg
import mpc_dealer as md
import oracle_lib as o
import prove_fs_cases as pc

pm = cg.pm
N = pm.N
pytestmark = pytest.mark.gpu
CAP = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOT_LANE_MAX = 16      # PROVE_FS_DOT_LANE_MAX (csrc/kernels.h): up to this m a proof's lane sums <wV, v_blinding> itself, above it a block does
le, cut = md.le, md.cut


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gens(gpu):
    g = gpu.gens_create(o.gens("G", CAP), o.gens("H", CAP), o.generator(), o.generator(), 8)
    yield g
    gpu.gens_destroy(g)


class ModelGens:
    """the model's BulletproofGens interface over the oracle's generator chain"""

    def __init__(self, cap):
        self.gens_capacity = cap
        self._g = [pm.b2p(b) for b in cut(o.gens("G", cap), 64)]
        self._h = [pm.b2p(b) for b in cut(o.gens("H", cap), 64)]

    def G(self, n, share=0):
        return self._g[:n]

    def H(self, n, share=0):
        return self._h[:n]


@pytest.fixture(scope="module")
def mgens():
    return ModelGens(16)


# (n, m, q, nb, profile)
SHAPES = [(1, 1, 1, 1, "dense"), (2, 0, 3, 2, "sparse"), (3, 2, 7, 3, "sparse"), (5, 5, 12, 3, "dups+holes"),
          (8, 1, 40, 2, "columns+edge_coeff"), (13, 11, 70, 1, "dense")]
_cache = {}


def case(mgens, shape, vkeys, sample=None):
    """the circuit of a shape and the model's records of its batch (computed once); sample: only these proofs of the batch"""
    n, m, q, nb, profile = shape
    key = (shape, vkeys, sample)
    if key not in _cache:
        circ = cg.Circuit(500 + 10 * n + m, n, 0, m, q, 0, profile)
        _cache[key] = (circ, {p: pc.model_proof(circ, mgens, p, vkeys, 500 + n) for p in (sample or range(nb))})
    return _cache[key]


def make(gpu, circ):
    return gpu.circuit_create(*circ.csr(), circ.n, circ.m)


def proof_slice(out, nb, k, p):
    pts, sc, wire, ch, so = out
    nvar, plen = 11 + 2 * k, 1 + 11 * 32 + (2 * k + 2) * 32
    return (pts[64 * nvar * p:64 * nvar * (p + 1)], sc[160 * p:160 * (p + 1)], wire[plen * p:plen * (p + 1)],
            ch[32 * (5 + k) * p:32 * (5 + k) * (p + 1)], so[32 * p:32 * (p + 1)])


def expected(r):
    return r["points"], r["scalars"], r["wire"], r["challenges"], r["state_out"]


# ------------------------------------------------------------------------------------------------ 1, 2: bytes, wire, round trip
@pytest.mark.parametrize("vkeys", (False, True))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-m%d-q%d-nb%d" % s[:4])
def test_fused_proofs_equal_the_model(gpu, gens, mgens, shape, vkeys):
    """proof_points, proof_scalars, wire, challenges_out and states_out of every proof of the batch are the model's bytes"""
    n, m, q, nb, _ = shape
    circ, recs = case(mgens, shape, vkeys)
    h = make(gpu, circ)
    try:
        out = gpu.r1cs_prove_fs(gens, h, nb, n, m, **pc.operands([recs[p] for p in range(nb)], vkeys))
    finally:
        gpu.circuit_destroy(h)
    k = pc.lg_padded(n)
    for p in range(nb):
        got, want = proof_slice(out, nb, k, p), expected(recs[p])
        for name, g, w in zip(("points", "scalars", "wire", "challenges", "state"), got, want):
            assert g == w, (name, p)


def test_first_and_last_proof_of_seventy(gpu, gens, mgens):
    """a second 64-lane block of every per-proof launch: 70 provers (the circuit's witness under 70 labels and blinding sets; the model
    proves the first and the last one, the others take blindings of the same generator)"""
    shape, nb = (3, 2, 7, 70, "sparse"), 70
    n, m = shape[:2]
    circ, recs = case(mgens, shape, False, sample=(0, 69))
    rnd = random.Random(70)
    filler = dict(recs[0])
    batch = []
    for p in range(nb):
        if p in recs:
            batch.append(recs[p])
        else:
            r = dict(filler)
            r["state_in"] = bytes(rnd.getrandbits(8) for _ in range(32))
            r["blindings"] = b"".join(md.mont(rnd.randrange(N)) for _ in range(8))
            batch.append(r)
    h = make(gpu, circ)
    try:
        out = gpu.r1cs_prove_fs(gens, h, nb, n, m, **pc.operands(batch, False))
    finally:
        gpu.circuit_destroy(h)
    for p in (0, 69):
        assert proof_slice(out, nb, pc.lg_padded(n), p) == expected(recs[p]), p


def with_commitments(points, V, nb, k):
    """the verifier's operand layout: V_0..V_{m-1} inserted after the six A / S points of each proof"""
    nvar, out = 11 + 2 * k, b""
    for p in range(nb):
        pp = points[64 * nvar * p:64 * nvar * (p + 1)]
        out += pp[:6 * 64] + b"".join(pm.p2b(v) for v in V[p]) + pp[6 * 64:]
    return out


@pytest.mark.parametrize("shape", (SHAPES[2], SHAPES[3]), ids=("n3", "n5"))
def test_wire_and_round_trip_through_the_verifiers(gpu, gens, mgens, shape):
    """the GPU's proofs verify: from their wire bytes (bpgpu_r1cs_verify_batch_wire), from points and scalars with the device transcript
    (bpgpu_r1cs_verify_batch_fs) and under the model's Verifier.verify; one flipped bit of t_x and all three reject"""
    n, m, q, nb, _ = shape
    circ, recs = case(mgens, shape, False)
    k = pc.lg_padded(n)
    plen = 1 + 11 * 32 + (2 * k + 2) * 32
    h = make(gpu, circ)
    try:
        pts, sc, wire, ch, so = gpu.r1cs_prove_fs(gens, h, nb, n, m, **pc.operands([recs[p] for p in range(nb)], False))
        assert wire == b"".join(pm.r1cs_proof_to_bytes(recs[p]["proof"]) for p in range(nb))
        init = b"".join(pm.Transcript(pc.label(p)).state for p in range(nb))
        V = [recs[p]["V"] for p in range(nb)]
        com = b"".join(pm.point_compress(v) for p in range(nb) for v in V[p])
        assert gpu.r1cs_verify_batch_wire(gens, h, nb, n, plen, wire, com, init) == [1] * nb
        assert gpu.r1cs_verify_batch_fs(gens, h, nb, n, k, m, init, with_commitments(pts, V, nb, k), sc)[0] == [1] * nb
        # t_x of proof 1: big-endian on the wire (its last byte is the low one), little-endian in proof_scalars
        bad_wire = bytearray(wire)
        bad_wire[plen + 1 + 8 * 32 + 31] ^= 4
        bad_sc = bytearray(sc)
        bad_sc[160] ^= 4
        want = [1, 0] + [1] * (nb - 2)
        assert gpu.r1cs_verify_batch_wire(gens, h, nb, n, plen, bytes(bad_wire), com, init) == want
        assert gpu.r1cs_verify_batch_fs(gens, h, nb, n, k, m, init, with_commitments(pts, V, nb, k), bytes(bad_sc))[0] == want
    finally:
        gpu.circuit_destroy(h)
    for p in range(nb):
        proof = pm.r1cs_proof_from_bytes(wire[plen * p:plen * (p + 1)])
        vf = pm.Verifier(pm.PedersenGens(), pm.Transcript(pc.label(p)))
        circ.install(vf, commitments=V[p])
        assert vf.verify(proof, mgens), p
        if p == 1:
            vf = pm.Verifier(pm.PedersenGens(), pm.Transcript(pc.label(p)))
            circ.install(vf, commitments=V[p])
            assert not vf.verify(pm.r1cs_proof_from_bytes(bytes(bad_wire[plen * p:plen * (p + 1)])), mgens)


# ------------------------------------------------------------------------------------------------ 3: the two dot-product paths
@pytest.mark.parametrize("m", (DOT_LANE_MAX, DOT_LANE_MAX + 1, 300))
def test_t_x_blinding_on_both_dot_product_paths(gpu, gens, m):
    """t_x_blinding = sum_i tb_i x^i with tb2 = <wV, v_blinding> (prover.rs:644-660) from the returned x and z, on integers: m at the
    largest size a lane sums by itself, the first size a block sums, and a few hundred terms (more than one pass of the block)"""
    n, nb = 2, 3
    circ = cg.Circuit(900 + m, n, 0, m, 9, 0, "dense")
    rnd = random.Random(m)
    vb = [[rnd.randrange(N) for _ in range(m)] for _ in range(nb)]
    bl = [[rnd.randrange(N) for _ in range(8)] for _ in range(nb)]
    wit = lambda v: b"".join(md.mont(x) for x in v) * nb      # noqa: E731
    h = make(gpu, circ)
    try:
        pts, sc, wire, ch, so = gpu.r1cs_prove_fs(
            gens, h, nb, n, m, states=bytes(rnd.getrandbits(8) for _ in range(32 * nb)), a_L=wit(circ.a_L[:n]), a_R=wit(circ.a_R[:n]),
            a_O=wit([circ.a_L[i] * circ.a_R[i] for i in range(n)]), blindings=b"".join(md.mont(x) for b in bl for x in b),
            v_blinding=b"".join(md.mont(x) for v in vb for x in v), vector_keys=bytes(rnd.getrandbits(8) for _ in range(32 * nb)),
            want_wire=False)
    finally:
        gpu.circuit_destroy(h)
    k = pc.lg_padded(n)
    for p in range(nb):
        c = [int.from_bytes(b, "little") for b in cut(ch[32 * (5 + k) * p:32 * (5 + k) * (p + 1)], 32)]
        z, x = c[1], c[3]
        wV = cg.model_weights(circ, z)[3]
        tb2 = sum(a * b for a, b in zip(wV, vb[p])) % N
        tb = [bl[p][3], tb2] + bl[p][4:]
        want = sum(t * pow(x, i + 1, N) for i, t in enumerate(tb)) % N
        assert int.from_bytes(sc[160 * p + 32:160 * p + 64], "little") == want, p


# ------------------------------------------------------------------------------------------------ 4: device form
def test_dev_form_equals_the_host_form_and_flags_a_bad_limb(gpu, gens, mgens):
    import mpc_bulletproof_amd as mm
    shape = SHAPES[3]
    n, m, q, nb, _ = shape
    circ, recs = case(mgens, shape, True)
    kw = pc.operands([recs[p] for p in range(nb)], True)
    k = pc.lg_padded(n)
    sizes = (64 * nb * (11 + 2 * k), 160 * nb, nb * (1 + 11 * 32 + (2 * k + 2) * 32), 32 * nb * (5 + k), 32 * nb)
    h = make(gpu, circ)
    bufs = []
    try:
        host = gpu.r1cs_prove_fs(gens, h, nb, n, m, **kw)
        d = {name: gpu.to_device(v) for name, v in kw.items()}
        outs = [gpu.malloc(s) for s in sizes]
        bufs = list(d.values()) + outs

        def run():
            gpu.r1cs_prove_fs_dev(gens, h, nb, d["states"], d["a_L"], d["a_R"], d["a_O"], d["blindings"], outs[0], outs[1],
                                  d_v_blinding=d["v_blinding"], d_vector_keys=d["vector_keys"], d_wire=outs[2], d_ch=outs[3],
                                  d_states_out=outs[4])
        run()
        assert gpu.input_flag() == 0
        assert tuple(gpu.download(p, s) for p, s in zip(outs, sizes)) == host
        # a_R[1] := the group order: not a canonical limb set
        bad = kw["a_R"][:32] + N.to_bytes(32, "little") + kw["a_R"][64:]
        gpu.upload(d["a_R"], bad)
        run()
        assert gpu.input_flag() == 1
        with pytest.raises(mm.lib.BpGpuError) as e:
            gpu.r1cs_prove_fs(gens, h, nb, n, m, **dict(kw, a_R=bad))
        assert e.value.code == mm.lib.E_ARG
        assert gpu.r1cs_prove_fs(gens, h, nb, n, m, **kw) == host
    finally:
        for b in bufs:
            gpu.free(b)
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ 5: the staged sequence
@pytest.mark.parametrize("vkeys", (False, True))
def test_staged_entry_points_give_the_same_bytes(gpu, gens, mgens, vkeys):
    """commit -> session_polys -> msm_gens -> ipp_begin -> run_fs with the challenges the fused call returned"""
    shape = SHAPES[3]
    n, m, q, nb, _ = shape
    circ, recs = case(mgens, shape, vkeys)
    rl = [recs[p] for p in range(nb)]
    kw = pc.operands(rl, vkeys)
    k, np_ = pc.lg_padded(n), 1 << pc.lg_padded(n)
    nvar = 11 + 2 * k
    h = make(gpu, circ)
    sess = ipp = None
    try:
        pts, sc, wire, ch, so = gpu.r1cs_prove_fs(gens, h, nb, n, m, **kw)
        chal = [cut(ch[32 * (5 + k) * p:32 * (5 + k) * (p + 1)], 32) for p in range(nb)]
        col = lambda j: b"".join(c[j] for c in chal)      # noqa: E731
        bl = cut(kw["blindings"], 32)
        sess, A = gpu.r1cs_prover_commit(gens, None, nb, n, kw["a_L"], kw["a_R"], kw["a_O"],
                                         b"".join(b"".join(bl[8 * p:8 * p + 3]) for p in range(nb)), kw.get("s_L"), kw.get("s_R"),
                                         kw.get("vector_keys"))
        t, wV = gpu.r1cs_prover_session_polys(sess, h, nb, m, col(0), col(1))
        tc = cut(t, 32)
        rows = b""
        for p in range(nb):
            for j, ti in enumerate((0, 2, 3, 4, 5)):
                tb = int.from_bytes(bl[8 * p + 3 + j], "little") * pow(1 << 256, -1, N) % N      # ark form -> canonical
                rows += tc[6 * p + ti] + le(tb)
        T = gpu.msm_gens(gens, nb * 5, 0, rows)
        ipp = gpu.r1cs_prover_ipp_begin(sess, gens, np_, n, col(3), col(2), None, col(4))
        # the chain states after innerproduct_domain_sep, replayed with the model's transcript from the fused call's own outputs
        st = b""
        for p in range(nb):
            tr = pm.Transcript(b"")
            tr.state = rl[p]["state_in"]
            tr.append_u64(b"m", m)
            pp = cut(pts[64 * nvar * p:64 * nvar * (p + 1)], 64)
            for lab, x in zip((b"A_I1", b"A_O1", b"S1"), pp[:3]):
                tr.append_message(lab, x)
            tr.r1cs_1phase_domain_sep()
            for lab in (b"A_I2", b"A_O2", b"S2"):
                tr.append_message(lab, bytes(64))
            assert [le(tr.challenge_scalar(b"y")), le(tr.challenge_scalar(b"z"))] == chal[p][:2]
            for lab, x in zip((b"T_1", b"T_3", b"T_4", b"T_5", b"T_6"), pp[6:11]):
                tr.append_message(lab, x)
            assert [le(tr.challenge_scalar(b"u")), le(tr.challenge_scalar(b"x"))] == chal[p][2:4]
            for lab, x in zip((b"t_x", b"t_x_blinding", b"e_blinding"), cut(sc[160 * p:160 * p + 96], 32)):
                tr.append_message(lab, x)
            assert le(tr.challenge_scalar(b"w")) == chal[p][4]
            tr.innerproduct_domain_sep(np_)
            st += tr.state
        L, R, a, b, so2 = gpu.ipp_run_fs(ipp, nb, k, st)
        for p in range(nb):
            want = A[192 * p:192 * (p + 1)] + bytes(192) + T[320 * p:320 * (p + 1)] + L[64 * k * p:64 * k * (p + 1)] + R[64 * k * p:64 * k * (p + 1)]
            assert pts[64 * nvar * p:64 * nvar * (p + 1)] == want, p
            assert sc[160 * p + 96:160 * (p + 1)] == a[32 * p:32 * (p + 1)] + b[32 * p:32 * (p + 1)], p
        assert so == so2
    finally:
        if ipp is not None:
            gpu.ipp_destroy(ipp)
        if sess is not None:
            gpu.prover_destroy(sess)
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_leave_the_context_usable(gpu, gens, mgens):
    import mpc_bulletproof_amd as mm
    E = mm.lib
    shape = SHAPES[0]
    n, m, q, nb, _ = shape
    circ, recs = case(mgens, shape, False)
    kw = pc.operands([recs[0]], False)
    keys = pc.operands([recs[0]], True)["vector_keys"]
    par = cg.Circuit(6, 2, 1, 1, 4, 1, "sparse")
    empty = cg.Circuit(7, 0, 0, 1, 1, 0, "sparse")
    wide = cg.Circuit(8, CAP + 1, 0, 0, 3, 0, "sparse")
    h = make(gpu, circ)
    hp = gpu.circuit_create_param(par.q, par.nchi, *par.csr_param(), par.n, par.m)
    he, hw = make(gpu, empty), make(gpu, wide)
    big = bytes(32 * 8 * (CAP + 1))

    def code(handle, nn, mmm, **over):
        try:
            gpu.r1cs_prove_fs(gens, handle, 1, nn, mmm, **dict(kw, **over))
        except E.BpGpuError as e:
            return e.code
        return 0
    try:
        for name in ("states", "a_L", "a_R", "a_O", "blindings", "v_blinding"):
            assert code(h, n, m, **{name: None}) == E.E_ARG, name
        assert code(h, n, m, s_L=None) == E.E_ARG and code(h, n, m, s_R=None) == E.E_ARG
        assert code(h, n, m, s_L=None, s_R=None) == E.E_ARG                      # neither source
        assert code(h, n, m, vector_keys=keys) == E.E_ARG                        # both
        assert code(hp, par.n, par.m) == E.E_ARG                                 # a parametric circuit
        assert code(he, 0, 1) == E.E_LEN                                         # no multipliers
        assert code(hw, CAP + 1, 0, a_L=big, a_R=big, a_O=big, s_L=big, s_R=big, v_blinding=None) == E.E_GENS
        gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, C.c_size_t(0), C.c_size_t(2)))
        try:
            assert code(h, n, m) == E.E_ARG
        finally:
            gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, C.c_size_t(0), C.c_size_t(1)))
        assert E._lib.bpgpu_r1cs_prove_fs(gpu.ctx, gens, h, C.c_size_t(0), *([None] * 14)) == 0      # nb == 0
        out = gpu.r1cs_prove_fs(gens, h, 1, n, m, **kw)
        assert proof_slice(out, 1, 0, 0) == expected(recs[0])
    finally:
        for x in (h, hp, he, hw):
            gpu.circuit_destroy(x)


# ------------------------------------------------------------------------------------------------ 7: the host mirror
def _host_prove(host, kind, param, label, values, seed, cap):
    vals = (C.c_uint64 * max(len(values), 1))(*values)
    proof = (C.c_uint8 * 8192)()
    plen, m = C.c_size_t(0), C.c_size_t(0)
    com = (C.c_uint8 * (64 * max(1, 2 * param if kind == o.K_SHUFFLE else param >> 16, 5)))()
    rc = host.bph_r1cs_prove(kind, C.c_size_t(param), o._buf(label), C.c_size_t(len(label)), vals, C.c_size_t(len(values)),
                             C.c_uint64(seed), C.c_size_t(cap), proof, C.byref(plen), com, C.byref(m))
    return rc, bytes(proof)[:plen.value], bytes(com)[:64 * m.value]


def test_host_mirror_takes_the_fused_call(monkeypatch):
    """BPH_PROVE_FUSED: Prover::prove_batch through bpgpu_r1cs_prove_fs gives the oracle's proof bytes, in both blinding modes; a
    two-phase circuit (the shuffle) keeps the staged route"""
    monkeypatch.setenv("BPH_PROVE_FUSED", "1")
    host = C.CDLL(os.path.join(ROOT, "tests", "host", "libbph_capi.so"))
    rnd = random.Random(7)
    cases = [(o.K_RANGE, w, [rnd.getrandbits(w)]) for w in (1, 7, 33, 64)]
    cases.append((o.K_RANGE_MULTI, 8 | (3 << 16), [rnd.getrandbits(8) for _ in range(3)]))
    xs = [rnd.getrandbits(64) for _ in range(3)]
    cases.append((o.K_SHUFFLE, 3, xs + xs[::-1]))
    for vkeys in (0, 1):
        host.bph_set_seeded_vector_keys(vkeys)
        try:
            for kind, param, values in cases:
                seed, cap, label = rnd.getrandbits(48), 128, b"fused prover %d" % param
                rc_o, proof_o, com_o = o.r1cs_prove(kind, param, label, values, seed, cap, vector_keys=bool(vkeys))
                rc, proof, com = _host_prove(host, kind, param, label, values, seed, cap)
                assert rc == rc_o == 0 and proof == proof_o and com == com_o, (kind, param, vkeys)
        finally:
            host.bph_set_seeded_vector_keys(0)
