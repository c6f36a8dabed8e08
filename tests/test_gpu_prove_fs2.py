"""bpgpu_r1cs_prove_fs2_begin / _finish -- Prover::prove of a two-phase circuit in two device calls around the gadget, transcript
included -- against the Python model (oracle/pymodel.py: Prover.prove under a replay RNG, tests/prove_fs2_cases.py) on generated
circuits and on the k-shuffle, against the staged entry points, against the verifiers (bpgpu_r1cs_verify_batch_wire2 among them), and
through the host mirror (BPH_PROVE_FUSED).  Run with `-m gpu` on an MI355X."""
import ctypes as C
import os
import random

import pytest

import circuit_gen as cg
import mpc_dealer as md
import oracle_lib as o
import prove_fs2_cases as pc
import prove_fs_cases as pc1

pm = cg.pm
N = pm.N
pytestmark = pytest.mark.gpu
CAP = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
le, cut = md.le, md.cut
EXPLICIT, KEYS, MIXED = (False, False), (True, True), (True, False)
SHUFFLE_LABEL = b"shuffle challenge"


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


# provers per shape (the model takes 1-3 s per proof)
NB = {pc.SHAPES[0]: 1, pc.SHAPES[1]: 3, pc.SHAPES[2]: 2, pc.SHAPES[3]: 2, pc.SHAPES[4]: 2, pc.SHAPES[5]: 2, pc.SHAPES[6]: 1}
S_PAD3 = pc.SHAPES[3]
_circuits, _records = {}, {}


def circuit(shape):
    if shape not in _circuits:
        _circuits[shape] = pc.circuit(shape)
    return _circuits[shape]


def records(mgens, shape, vkeys, proofs):
    """the model's records of proofs `proofs` of a shape's batch (each computed once and left unchanged)"""
    circ = circuit(shape)
    for p in proofs:
        if (shape, vkeys, p) not in _records:
            _records[(shape, vkeys, p)] = pc.model_proof(circ, mgens, p, vkeys, 700 + shape[0])
    return circ, [_records[(shape, vkeys, p)] for p in proofs]


def make(gpu, circ):
    return gpu.circuit_create_param(circ.q, 1, *circ.csr_param(), circ.n, circ.m)


def prove(gpu, gens, h, circ, recs, vkeys):
    """both calls on a batch of records -> (commitments, chi, states after the challenge), (points, scalars, wire, challenges, states)"""
    nb = len(recs)
    sess, com, chi, st = gpu.r1cs_prove_fs2_begin(gens, h, nb, circ.n1, gadget_label=cg.CHI_LABEL, **pc.begin_operands(recs, vkeys, circ.n1))
    assert sess is not None
    out = gpu.r1cs_prove_fs2_finish(gens, h, sess, nb, circ.n, circ.m, **pc.finish_operands(recs, vkeys))
    assert not sess.value                  # consumed
    return (com, chi, st), out


def proof_slice(out, k, p):
    pts, sc, wire, ch, so = out
    nvar, plen = 11 + 2 * k, 1 + 14 * 32 + (2 * k + 2) * 32
    return (pts[64 * nvar * p:64 * nvar * (p + 1)], sc[160 * p:160 * (p + 1)], wire[plen * p:plen * (p + 1)],
            ch[32 * (5 + k) * p:32 * (5 + k) * (p + 1)], so[32 * p:32 * (p + 1)])


def expected(r):
    return r["points"], r["scalars"], r["wire"], r["challenges"], r["state_out"]


def check_against_model(first, out, recs, k, which=None):
    com, chi, st = first
    for p in (which if which is not None else range(len(recs))):
        r = recs[p]
        assert com[192 * p:192 * (p + 1)] == r["commitments"], ("commitments", p)
        assert chi[32 * p:32 * (p + 1)] == r["chi"], ("gadget challenge", p)
        assert st[32 * p:32 * (p + 1)] == r["state_mid"], ("state after the gadget challenge", p)
        for name, g, w in zip(("points", "scalars", "wire", "challenges", "state"), proof_slice(out, k, p), expected(r)):
            assert g == w, (name, p)


# ------------------------------------------------------------------------------------------------ 1: the model's bytes
CASES = [(s, EXPLICIT) for s in pc.SHAPES] + [(pc.SHAPES[2], KEYS), (S_PAD3, KEYS), (pc.SHAPES[2], MIXED)]


@pytest.mark.parametrize("shape,vkeys", CASES, ids=lambda v: "n%d+%d-m%d-q%d" % v[:4] if len(v) == 5 else "keys%d%d" % v)
def test_two_call_proofs_equal_the_model(gpu, gens, mgens, shape, vkeys):
    """commitments, the gadget challenge, proof_points, proof_scalars, wire, challenges_out and both states_out of every proof of the
    batch are the model's bytes; the wire form is version 1 with all 14 points"""
    nb = NB[shape]
    circ, recs = records(mgens, shape, vkeys, range(nb))
    h = make(gpu, circ)
    try:
        first, out = prove(gpu, gens, h, circ, recs, vkeys)
    finally:
        gpu.circuit_destroy(h)
    k = pc.lg_padded(circ.n)
    assert len(out[2]) == nb * (1 + 14 * 32 + (2 * k + 2) * 32) and out[2][0] == 1
    check_against_model(first, out, recs, k)


# ------------------------------------------------------------------------------------------------ 2: seventy provers
def test_first_and_last_proof_of_seventy(gpu, gens, mgens):
    """a second 64-lane block of every per-proof launch: 70 provers (the circuit's witness, which satisfies it for every challenge,
    under 70 labels and blinding sets; the model proves the first and the last one, the others take blindings of the same generator)"""
    nb = 70
    circ, (r0, r69) = records(mgens, S_PAD3, EXPLICIT, (0, 69))
    rnd = random.Random(70)
    batch = []
    for p in range(nb):
        if p in (0, 69):
            batch.append(r0 if p == 0 else r69)
        else:
            r = dict(r0)
            r["state_in"] = bytes(rnd.getrandbits(8) for _ in range(32))
            r["bl1"] = b"".join(md.mont(rnd.randrange(N)) for _ in range(3))
            r["bl2"] = b"".join(md.mont(rnd.randrange(N)) for _ in range(8))
            batch.append(r)
    h = make(gpu, circ)
    try:
        first, out = prove(gpu, gens, h, circ, batch, EXPLICIT)
    finally:
        gpu.circuit_destroy(h)
    check_against_model(first, out, batch, pc.lg_padded(circ.n), which=(0, 69))


# ------------------------------------------------------------------------------------------------ 3: a witness that depends on the challenge
def with_commitments(points, V, nb, k):
    """the verifier's operand layout: V_0..V_{m-1} inserted after the six A / S points of each proof"""
    nvar, out = 11 + 2 * k, b""
    for p in range(nb):
        pp = points[64 * nvar * p:64 * nvar * (p + 1)]
        out += pp[:6 * 64] + b"".join(pm.p2b(v) for v in V[p]) + pp[6 * 64:]
    return out


def _shuffle_prover(p, ks, seed):
    """a model prover of the ks-shuffle after its commitments and the gadget's first phase -> (prover, commitments, v_blinding)"""
    r = random.Random(seed * 100 + p)
    xs = [r.getrandbits(40) for _ in range(ks)]
    ys = list(xs)
    r.shuffle(ys)
    vb = [r.randrange(N) for _ in range(2 * ks)]
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(pc.label(p)))
    cv = [pv.commit(v, b) for v, b in zip(xs + ys, vb)]
    pm.shuffle_gadget(pv, [c[1] for c in cv[:ks]], [c[1] for c in cv[ks:]])
    return pv, [c[0] for c in cv], vb


@pytest.mark.parametrize("ks", (2, 4))
def test_shuffle_witness_is_evaluated_on_the_returned_challenge(gpu, gens, mgens, ks):
    """the k-shuffle (tests/r1cs.rs:23-62; no phase-1 multipliers, 2 (k - 1) in phase 2): _begin returns the model's challenge, the
    test evaluates the gadget with it, _finish gives the model's proof bytes; bpgpu_r1cs_verify_batch_fs2, bpgpu_r1cs_verify_batch_wire2
    and the model's Verifier accept; with one flipped bit of t_x in proof 1 all three reject that proof and only that one"""
    nb, seed = 2, 40 + ks
    n, m = 2 * (ks - 1), 2 * ks
    k = pc.lg_padded(n)
    nvar, plen = 11 + 2 * k, 1 + 14 * 32 + (2 * k + 2) * 32
    rnd = random.Random(seed)
    ark = lambda v: b"".join(map(md.mont, v))      # noqa: E731
    model, draws, V, vbs = [], [], [], []
    for p in range(nb):
        pv, Vp, vb = _shuffle_prover(p, ks, seed)
        d = dict(bl1=[rnd.randrange(N) for _ in range(3)], bl2=[rnd.randrange(N) for _ in range(3)], sL=[rnd.randrange(N) for _ in range(n)],
                 sR=[rnd.randrange(N) for _ in range(n)], tb=[rnd.randrange(N) for _ in range(5)])
        rng = pc.Replay(d["bl1"] + d["bl2"] + d["sL"] + d["sR"] + d["tb"])
        proof = pv.prove(mgens, rng)
        assert not rng.values
        model.append((pv, proof))
        draws.append(d)
        V.append(Vp)
        vbs.append(vb)
    rp, kd, ix, cf, _ = md.circuit_rows(model[0][0].constraints, param=True)
    h = gpu.circuit_create_param(len(model[0][0].constraints), 1, rp, kd, ix, cf, n, m)
    try:
        twins = [_shuffle_prover(p, ks, seed)[0] for p in range(nb)]
        sess, com, chi, st = gpu.r1cs_prove_fs2_begin(gens, h, nb, 0, states=b"".join(t.transcript.state for t in twins),
                                                      gadget_label=SHUFFLE_LABEL, blindings=b"".join(ark(d["bl1"]) for d in draws))
        for p, tw in enumerate(twins):
            assert chi[32 * p:32 * (p + 1)] == le(md.circuit_rows(model[p][0].constraints, param=True)[4]), p
            z = int.from_bytes(chi[32 * p:32 * (p + 1)], "little")
            tw.challenge_scalar = lambda label, z=z: z          # the gadget runs on the DEVICE's challenge
            tw._create_randomized_constraints()
            assert len(tw.a_L) == n
        pts, sc, wire, ch, so = gpu.r1cs_prove_fs2_finish(
            gens, h, sess, nb, n, m, a_L=b"".join(ark(t.a_L) for t in twins), a_R=b"".join(ark(t.a_R) for t in twins),
            a_O=b"".join(ark(t.a_O) for t in twins), s_L=b"".join(ark(d["sL"]) for d in draws), s_R=b"".join(ark(d["sR"]) for d in draws),
            blindings=b"".join(ark(d["bl2"] + d["tb"]) for d in draws), v_blinding=b"".join(ark(v) for v in vbs))
        assert wire == b"".join(pm.r1cs_proof_to_bytes(proof) for _, proof in model)
        assert so == b"".join(pv.transcript.state for pv, _ in model)
        init = b"".join(pm.Transcript(pc.label(p)).state for p in range(nb))
        cmp_ = b"".join(pm.point_compress(v) for p in range(nb) for v in V[p])
        full = with_commitments(pts, V, nb, k)
        assert gpu.r1cs_verify_batch_fs2(gens, h, nb, 0, k, m, 1, init, SHUFFLE_LABEL, full, sc)[0] == [1] * nb
        assert gpu.r1cs_verify_batch_wire2(gens, h, nb, 0, plen, SHUFFLE_LABEL, wire, cmp_, init) == [1] * nb
        # t_x of proof 1: big-endian on the wire (slot 11 of version 1; its last byte is the low one), little-endian in proof_scalars
        bad_wire = bytearray(wire)
        bad_wire[plen + 1 + 11 * 32 + 31] ^= 4
        bad_sc = bytearray(sc)
        bad_sc[160] ^= 4
        assert gpu.r1cs_verify_batch_fs2(gens, h, nb, 0, k, m, 1, init, SHUFFLE_LABEL, full, bytes(bad_sc))[0] == [1, 0]
        assert gpu.r1cs_verify_batch_wire2(gens, h, nb, 0, plen, SHUFFLE_LABEL, bytes(bad_wire), cmp_, init) == [1, 0]
    finally:
        gpu.circuit_destroy(h)

    def model_accepts(p, proof_bytes):
        vf = pm.Verifier(pm.PedersenGens(), pm.Transcript(pc.label(p)))
        vars_ = [vf.commit(v) for v in V[p]]
        pm.shuffle_gadget(vf, vars_[:ks], vars_[ks:])
        return bool(vf.verify(pm.r1cs_proof_from_bytes(proof_bytes), mgens))
    assert [model_accepts(p, wire[plen * p:plen * (p + 1)]) for p in range(nb)] == [True] * nb
    assert not model_accepts(1, bytes(bad_wire[plen:2 * plen]))


# ------------------------------------------------------------------------------------------------ 4: the staged sequence
@pytest.mark.parametrize("vkeys", (EXPLICIT, KEYS), ids=("explicit", "keys"))
def test_staged_entry_points_give_the_same_bytes(gpu, gens, mgens, vkeys):
    """commit, commit -> session_polys_param -> msm_gens -> ipp_begin -> run_fs with the challenges the two calls returned"""
    shape = S_PAD3
    nb = NB[shape]
    circ, recs = records(mgens, shape, vkeys, range(nb))
    n1, n, m = circ.n1, circ.n, circ.m
    k, np_ = pc.lg_padded(n), 1 << pc.lg_padded(n)
    nvar = 11 + 2 * k
    b1, b2 = pc.begin_operands(recs, vkeys, n1), pc.finish_operands(recs, vkeys)
    h = make(gpu, circ)
    sess = ipp = None
    try:
        (com, chi, st_mid), (pts, sc, wire, ch, so) = prove(gpu, gens, h, circ, recs, vkeys)
        chal = [cut(ch[32 * (5 + k) * p:32 * (5 + k) * (p + 1)], 32) for p in range(nb)]
        col = lambda j: b"".join(c[j] for c in chal)      # noqa: E731
        bl = cut(b2["blindings"], 32)
        sess, A1 = gpu.r1cs_prover_commit(gens, None, nb, n1, b1["a_L"], b1["a_R"], b1["a_O"], b1["blindings"], b1.get("s_L"), b1.get("s_R"),
                                          b1.get("vector_keys"))
        sess, A2 = gpu.r1cs_prover_commit(gens, sess, nb, n - n1, b2["a_L"], b2["a_R"], b2["a_O"],
                                          b"".join(b"".join(bl[8 * p:8 * p + 3]) for p in range(nb)), b2.get("s_L"), b2.get("s_R"),
                                          b2.get("vector_keys"))
        assert A1 == com
        t, wV = gpu.r1cs_prover_session_polys_param(sess, h, nb, m, col(0), col(1), chi)
        tc = cut(t, 32)
        rows = b""
        for p in range(nb):
            for j, ti in enumerate((0, 2, 3, 4, 5)):
                tb = int.from_bytes(bl[8 * p + 3 + j], "little") * pow(1 << 256, -1, N) % N      # ark form -> canonical
                rows += tc[6 * p + ti] + le(tb)
        T = gpu.msm_gens(gens, nb * 5, 0, rows)
        ipp = gpu.r1cs_prover_ipp_begin(sess, gens, np_, n1, col(3), col(2), None, col(4))
        # the chain states after innerproduct_domain_sep, replayed with the model's transcript from the two calls' own outputs
        st = b""
        for p in range(nb):
            tr = pm.Transcript(b"")
            tr.state = st_mid[32 * p:32 * (p + 1)]
            pp = cut(pts[64 * nvar * p:64 * nvar * (p + 1)], 64)
            for lab, x in zip((b"A_I2", b"A_O2", b"S2"), pp[3:6]):
                tr.append_message(lab, x)
            assert [le(tr.challenge_scalar(b"y")), le(tr.challenge_scalar(b"z"))] == chal[p][:2]
            for lab, x in zip((b"T_1", b"T_3", b"T_4", b"T_5", b"T_6"), pp[6:11]):
                tr.append_message(lab, x)
            assert [le(tr.challenge_scalar(b"u")), le(tr.challenge_scalar(b"x"))] == chal[p][2:4]
            for lab, x in zip((b"t_x", b"t_x_blinding", b"e_blinding"), cut(sc[160 * p:160 * p + 96], 32)):
                tr.append_message(lab, x)
            assert le(tr.challenge_scalar(b"w")) == chal[p][4]
            tr.innerproduct_domain_sep(np_)
            st += tr.state
            # t_x = sum_i t_i x^i from the staged build's coefficients
            x = int.from_bytes(chal[p][3], "little")
            tx = sum(int.from_bytes(c, "little") * pow(x, i + 1, N) for i, c in enumerate(tc[6 * p:6 * p + 6])) % N
            assert sc[160 * p:160 * p + 32] == le(tx), p
        L, R, a, b, so2 = gpu.ipp_run_fs(ipp, nb, k, st)
        for p in range(nb):
            want = (A1[192 * p:192 * (p + 1)] + A2[192 * p:192 * (p + 1)] + T[320 * p:320 * (p + 1)] + L[64 * k * p:64 * k * (p + 1)] +
                    R[64 * k * p:64 * k * (p + 1)])
            assert pts[64 * nvar * p:64 * nvar * (p + 1)] == want, p
            assert sc[160 * p + 96:160 * (p + 1)] == a[32 * p:32 * (p + 1)] + b[32 * p:32 * (p + 1)], p
        assert so == so2
    finally:
        if ipp is not None:
            gpu.ipp_destroy(ipp)
        if sess is not None:
            gpu.prover_destroy(sess)
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ 5: device form
def test_dev_forms_back_to_back_equal_the_host_forms_and_flag_a_bad_limb(gpu, gens, mgens):
    """_begin_dev and _finish_dev enqueued one after the other, with no synchronise between them (the phase-2 witness is resident)"""
    import mpc_bulletproof_amd as mm
    shape, vkeys = S_PAD3, KEYS
    nb = NB[shape]
    circ, recs = records(mgens, shape, vkeys, range(nb))
    n1, n, m = circ.n1, circ.n, circ.m
    k = pc.lg_padded(n)
    b1, b2 = pc.begin_operands(recs, vkeys, n1), pc.finish_operands(recs, vkeys)
    sizes1 = (192 * nb, 32 * nb, 32 * nb)
    sizes2 = (64 * nb * (11 + 2 * k), 160 * nb, nb * (1 + 14 * 32 + (2 * k + 2) * 32), 32 * nb * (5 + k), 32 * nb)
    h = make(gpu, circ)
    bufs = []
    try:
        host1, host2 = prove(gpu, gens, h, circ, recs, vkeys)
        d1 = {name: gpu.to_device(v) for name, v in b1.items()}
        d2 = {name: gpu.to_device(v) for name, v in b2.items()}
        o1, o2 = [gpu.malloc(s) for s in sizes1], [gpu.malloc(s) for s in sizes2]
        bufs = list(d1.values()) + list(d2.values()) + o1 + o2

        def run():
            sess = gpu.r1cs_prove_fs2_begin_dev(gens, h, nb, n1, d1["states"], cg.CHI_LABEL, d1["blindings"], d_a_L=d1["a_L"], d_a_R=d1["a_R"],
                                                d_a_O=d1["a_O"], d_vector_keys=d1["vector_keys"], d_commitments=o1[0], d_chi=o1[1],
                                                d_states_out=o1[2])
            gpu.r1cs_prove_fs2_finish_dev(gens, h, sess, d2["a_L"], d2["a_R"], d2["a_O"], d2["blindings"], o2[0], o2[1],
                                          d_v_blinding=d2["v_blinding"], d_vector_keys=d2["vector_keys"], d_wire=o2[2], d_ch=o2[3],
                                          d_states_out=o2[4])
            assert not sess.value
        run()
        assert gpu.input_flag() == 0
        assert tuple(gpu.download(p, s) for p, s in zip(o1, sizes1)) == host1
        assert tuple(gpu.download(p, s) for p, s in zip(o2, sizes2)) == host2
        # a_R[1] of phase 2 := the group order: not a canonical limb set
        bad = b2["a_R"][:32] + N.to_bytes(32, "little") + b2["a_R"][64:]
        gpu.upload(d2["a_R"], bad)
        run()
        assert gpu.input_flag() == 1
        sess = gpu.r1cs_prove_fs2_begin(gens, h, nb, n1, gadget_label=cg.CHI_LABEL, **b1)[0]
        with pytest.raises(mm.lib.BpGpuError) as e:
            gpu.r1cs_prove_fs2_finish(gens, h, sess, nb, n, m, **dict(b2, a_R=bad))
        assert e.value.code == mm.lib.E_ARG and not sess.value      # launched: consumed all the same
        assert prove(gpu, gens, h, circ, recs, vkeys) == (host1, host2)
        gpu.upload(d2["a_R"], b2["a_R"])
        run()
        assert gpu.input_flag() == 0
        assert tuple(gpu.download(p, s) for p, s in zip(o2, sizes2)) == host2
    finally:
        for b in bufs:
            gpu.free(b)
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ 6: refusals and lifecycle
def test_refusals_and_the_session_lifecycle(gpu, gens, mgens):
    import mpc_bulletproof_amd as mm
    E = mm.lib
    shape = pc.SHAPES[2]                     # (1, 1, 1, 4)
    circ, recs = records(mgens, shape, EXPLICIT, (0,))
    n1, n, m = circ.n1, circ.n, circ.m
    b1, b2 = pc.begin_operands(recs, EXPLICIT, n1), pc.finish_operands(recs, EXPLICIT)
    keys = recs[0]["key1"]
    numeric = cg.Circuit(7, 2, 0, 1, 3, 0, "sparse")
    two_chi = cg.Circuit(8, 1, 1, 1, 4, 2, "sparse")
    wide = cg.Circuit(9, 1, CAP, 0, 4, 1, "sparse")
    h, h_other = make(gpu, circ), make(gpu, circ)
    hn = gpu.circuit_create(*numeric.csr(), numeric.n, numeric.m)
    h2 = gpu.circuit_create_param(two_chi.q, 2, *two_chi.csr_param(), two_chi.n, two_chi.m)
    hw = make(gpu, wide)
    open_ = []                               # sessions this test still owns

    def begin_code(handle, nn1=n1, **over):
        try:
            s = gpu.r1cs_prove_fs2_begin(gens, handle, 1, nn1, gadget_label=cg.CHI_LABEL, **dict(b1, **over))[0]
        except E.BpGpuError as e:
            return e.code
        open_.append(s)
        return 0

    def finish_code(handle, sess, **over):
        try:
            gpu.r1cs_prove_fs2_finish(gens, handle, sess, 1, n, m, **dict(b2, **over))
        except E.BpGpuError as e:
            return e.code
        return 0
    try:
        # ---- _begin
        for name in ("states", "blindings", "a_L", "a_R", "a_O"):
            assert begin_code(h, **{name: None}) == E.E_ARG, name
        assert begin_code(h, s_L=None) == E.E_ARG and begin_code(h, s_R=None) == E.E_ARG
        assert begin_code(h, s_L=None, s_R=None) == E.E_ARG                    # neither source
        assert begin_code(h, vector_keys=keys) == E.E_ARG                      # both
        assert begin_code(hn) == E.E_ARG                                       # a numeric circuit
        assert begin_code(h2) == E.E_ARG                                       # two gadget challenges
        assert begin_code(h, nn1=n) == E.E_LEN and begin_code(h, nn1=n + 1) == E.E_LEN      # no second phase
        assert begin_code(hw) == E.E_GENS
        taken = C.c_void_p(1)
        rc = E._lib.bpgpu_r1cs_prove_fs2_begin(gpu.ctx, gens, h, C.c_size_t(1), C.c_size_t(n1), b1["states"], cg.CHI_LABEL + bytes(6), b1["a_L"],
                                               b1["a_R"], b1["a_O"], b1["s_L"], b1["s_R"], None, b1["blindings"], C.byref(taken), None, None, None)
        assert rc == E.E_ARG and taken.value == 1                              # *session != NULL
        none = C.c_void_p()
        assert E._lib.bpgpu_r1cs_prove_fs2_begin(gpu.ctx, gens, h, C.c_size_t(0), C.c_size_t(n1), *([None] * 9), C.byref(none), None, None,
                                                 None) == 0 and not none.value  # nb == 0
        gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, C.c_size_t(0), C.c_size_t(2)))
        try:
            assert begin_code(h) == E.E_ARG
        finally:
            gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, C.c_size_t(0), C.c_size_t(1)))
        assert not open_
        # ---- an abandoned session
        assert begin_code(h) == 0
        gpu.prover_destroy(open_.pop())
        # ---- _finish's refusals leave the session open
        assert begin_code(h) == 0
        sess = open_[0]
        for name in ("a_L", "a_R", "a_O", "blindings", "v_blinding"):
            assert finish_code(h, sess, **{name: None}) == E.E_ARG and sess.value, name
        assert finish_code(h, sess, s_L=None) == E.E_ARG and finish_code(h, sess, s_L=None, s_R=None) == E.E_ARG
        assert finish_code(h, sess, vector_keys=recs[0]["key2"]) == E.E_ARG
        assert finish_code(h_other, sess) == E.E_ARG and sess.value            # another circuit handle
        gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, C.c_size_t(0), C.c_size_t(2)))
        try:
            assert finish_code(h, sess) == E.E_ARG and sess.value
        finally:
            gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, C.c_size_t(0), C.c_size_t(1)))
        assert finish_code(h, None) == E.E_ARG and finish_code(h, C.c_void_p()) == E.E_ARG      # no session
        # ---- the staged calls refuse a session of _begin
        with pytest.raises(E.BpGpuError) as e:
            gpu.r1cs_prover_commit(gens, sess, 1, n - n1, b2["a_L"], b2["a_R"], b2["a_O"], b2["blindings"][:96], b2["s_L"], b2["s_R"])
        assert e.value.code == E.E_ARG
        y = le(5)
        for call in (lambda: gpu.r1cs_prover_session_polys_param(sess, h, 1, m, y, y, y),
                     lambda: gpu.r1cs_prover_session_polys(sess, hn, 1, numeric.m, y, y),
                     lambda: gpu.r1cs_prover_eval(sess, 1, 2, y),
                     lambda: gpu.r1cs_prover_ipp_begin(sess, gens, 2, n1, y, y, y, y)):
            with pytest.raises(E.BpGpuError) as e:
                call()
            assert e.value.code == E.E_ARG
        # ... and after all of that the session still finishes, with the model's bytes
        out = gpu.r1cs_prove_fs2_finish(gens, h, sess, 1, n, m, **b2)
        assert not sess.value and proof_slice(out, pc.lg_padded(n), 0) == expected(recs[0])
        open_.pop()
        # ---- _finish refuses a staged session
        staged, _ = gpu.r1cs_prover_commit(gens, None, 1, n1, b1["a_L"], b1["a_R"], b1["a_O"], b1["blindings"], b1["s_L"], b1["s_R"])
        open_.append(staged)
        assert finish_code(h, staged) == E.E_ARG and staged.value
        gpu.prover_destroy(open_.pop())
        # ---- the context proves correctly afterwards
        first, out = prove(gpu, gens, h, circ, recs, EXPLICIT)
        check_against_model(first, out, recs, pc.lg_padded(n))
    finally:
        for s in open_:
            if s is not None and s.value:
                gpu.prover_destroy(s)
        for x in (h, h_other, hn, h2, hw):
            gpu.circuit_destroy(x)


# ------------------------------------------------------------------------------------------------ 7: both kinds on one context
# timed launches per profile kind (BpGpu.profile_read) of ONE call with nb = 1: bpgpu_r1cs_prove_fs on circuit A below,
# bpgpu_r1cs_prove_fs2_begin and _finish on circuit B -- the launch structure of each call
LAUNCHES_FS = dict(prover_commit=1, prover_polys=1, msm_gens=1, ipp_begin=1, ipp_rounds=1, ipp_round_msm=1, prove_fs_links=5)
LAUNCHES_BEGIN = dict(prover_commit=1, prove_fs_links=2)
LAUNCHES_FINISH = LAUNCHES_FS


def test_one_and_two_phase_proofs_alternate_on_one_context(gpu, gens, mgens):
    """the one-phase and the two-phase call share the context's transcript-schedule cache, workspace and chain: a one-phase circuit A
    (n = 2, m = 1) and a two-phase circuit B (n = 1 + 1, m = 1) have the SAME cache key (m, padded n) = (1, 2), A' (n = 2, m = 0) another.
    A, B, A again, A', then A between _begin and _finish of B: every call gives the model's bytes, and launches what it always did"""
    A, A_ = cg.Circuit(521, 2, 0, 1, 3, 0, "sparse"), cg.Circuit(520, 2, 0, 0, 3, 0, "sparse")
    rA, rA_ = pc1.model_proof(A, mgens, 0, False, 521), pc1.model_proof(A_, mgens, 0, False, 520)
    shape = pc.SHAPES[2]
    assert shape == (1, 1, 1, 4, "sparse")
    B, (rB,) = records(mgens, shape, EXPLICIT, (0,))
    assert (A.m, pc.lg_padded(A.n)) == (B.m, pc.lg_padded(B.n)) == (1, 1) and (A_.m, pc.lg_padded(A_.n)) == (0, 1)
    b1, b2 = pc.begin_operands([rB], EXPLICIT, B.n1), pc.finish_operands([rB], EXPLICIT)
    hA, hA_, hB = gpu.circuit_create(*A.csr(), A.n, A.m), gpu.circuit_create(*A_.csr(), A_.n, A_.m), make(gpu, B)
    open_ = []

    def launches():
        got = {name: cnt for name, (_, cnt) in gpu.profile_read().items() if cnt}
        print(got)
        return got

    def one_phase(h, circ, r):
        out = gpu.r1cs_prove_fs(gens, h, 1, circ.n, circ.m, **pc1.operands([r], False))
        got = launches()
        for name, g, w in zip(("points", "scalars", "wire", "challenges", "state"), out, expected(r)):
            assert g == w, name
        return out, got

    def begin():
        sess, com, chi, st = gpu.r1cs_prove_fs2_begin(gens, hB, 1, B.n1, gadget_label=cg.CHI_LABEL, **b1)
        open_.append(sess)
        return (com, chi, st), launches()

    def finish(first):
        out = gpu.r1cs_prove_fs2_finish(gens, hB, open_[0], 1, B.n, B.m, **b2)
        assert not open_.pop().value
        got = launches()
        check_against_model(first, out, [rB], pc.lg_padded(B.n))
        return got
    gpu.profile_enable(True)
    try:
        gpu.profile_read()
        out1, l1 = one_phase(hA, A, rA)                    # 1
        first, l2 = begin()                                # 2
        l3 = finish(first)
        out4, l4 = one_phase(hA, A, rA)                    # 3
        assert out4 == out1
        one_phase(hA_, A_, rA_)                            # 4
        first, l5 = begin()                                # 5
        out6, l6 = one_phase(hA, A, rA)                    # 6: B's session is open
        assert out6 == out1
        l7 = finish(first)                                 # 7
        assert l1 == l4 == l6 == LAUNCHES_FS
        assert l2 == l5 == LAUNCHES_BEGIN
        assert l3 == l7 == LAUNCHES_FINISH
    finally:
        gpu.profile_enable(False)
        for s in open_:
            if s is not None and s.value:
                gpu.prover_destroy(s)
        for h in (hA, hA_, hB):
            gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ 8: the host mirror
def _shuffle_prove_param(host, ks, values, seed, cap):
    arr = (C.c_uint64 * (2 * ks))(*values)
    proof, plen, com, ms3 = (C.c_uint8 * 8192)(), C.c_size_t(0), (C.c_uint8 * (2 * ks * 64))(), (C.c_double * 3)()
    rc = host.bph_shuffle_prove_param(C.c_size_t(ks), arr, C.c_uint64(seed), C.c_size_t(cap), proof, C.byref(plen), com, ms3)
    return rc, bytes(proof)[:plen.value], bytes(com)


@pytest.mark.parametrize("ks", (2, 5))
def test_host_mirror_takes_the_two_calls(monkeypatch, capfd, ks):
    """BPH_PROVE_FUSED: a prover bound to the shuffle's ParametricCircuit goes through bpgpu_r1cs_prove_fs2_begin / _finish and gives
    the oracle's proof bytes in both blinding modes; BPH_TIMING shows the two calls as laps, and neither without BPH_PROVE_FUSED"""
    host = C.CDLL(os.path.join(ROOT, "tests", "host", "libbph_capi.so"))
    rnd = random.Random(ks)
    xs = [rnd.getrandbits(64) for _ in range(ks)]
    values = xs + xs[::-1]
    monkeypatch.setenv("BPH_TIMING", "1")
    for vkeys in (0, 1):
        host.bph_set_seeded_vector_keys(vkeys)
        try:
            seed, cap = rnd.getrandbits(48), 128
            rc_o, proof_o, com_o = o.r1cs_prove(o.K_SHUFFLE, ks, b"ShuffleProofTest", values, seed, cap, vector_keys=bool(vkeys))
            for fused in (True, False):
                if fused:
                    monkeypatch.setenv("BPH_PROVE_FUSED", "1")
                else:
                    monkeypatch.delenv("BPH_PROVE_FUSED")
                capfd.readouterr()
                rc, proof, com = _shuffle_prove_param(host, ks, values, seed, cap)
                err = capfd.readouterr().err
                assert rc == rc_o == 0 and proof == proof_o and com == com_o, (ks, vkeys, fused)
                assert ("prove: fused begin" in err) == fused and ("prove: fused finish" in err) == fused, (ks, vkeys, fused, err)
        finally:
            host.bph_set_seeded_vector_keys(0)
