"""The two-party R1CS prover (src/r1cs_mpc/ of the reference) with each party's local arithmetic on its GPU (bpgpu_mpc_*): two parties
run on two contexts, the test plays the network (openings, MAC checks) and the transcript, and the opened proof must be the proof the
single-party prover makes from the same witness, blindings and transcript.  Run with `-m gpu` on an MI355X."""
import random

import pytest

import mpc_dealer as md
import oracle_lib as o

pytestmark = pytest.mark.gpu
pm = md.pm
N = md.N


@pytest.fixture(scope="module")
def gpus():
    import mpc_bulletproof_amd as m
    two = m.lib.device_count() >= 2
    g = [m.BpGpu(0), m.BpGpu(1 if two else 0)]
    yield g
    for x in g:
        x.close()


def _gens(gpus, cap):
    return [g.gens_create(o.gens("G", cap), o.gens("H", cap), o.generator(), o.generator(), 8) for g in gpus]


# ---- the model's provers: (oracle kind, param, label, values for the oracle's verifier) and a builder of the Prover after its
# commitments and phase-1 gadget, whose SplitMix64(seed) drew the v_blindings first (the CPU oracle's order)
def _range_prover(seed, nbits=8):
    rng = pm.SplitMix64(seed)
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"RangeProofTest"))
    v = (0x9E3779B97F4A7C15 * seed) % (1 << nbits)
    _, var = pv.commit(v, rng.scalar())
    pm.range_proof_gadget(pv, pm.lc_var(var), v, nbits)
    return pv, rng, (o.K_RANGE, nbits, b"RangeProofTest", [v])


def _example_prover(seed):
    rng = pm.SplitMix64(seed)
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"ExampleProofTest"))
    r = random.Random(seed)
    a1, a2, b1, b2 = (r.getrandbits(20) | 1 for _ in range(4))
    c2 = 1                                  # the constant is part of the circuit: one value for every proof of a batch
    c1 = (a1 + a2) * (b1 + b2) - c2
    vars_ = [pv.commit(v, rng.scalar())[1] for v in (a1, a2, b1, b2, c1)]
    pm.example_gadget(pv, *[pm.lc_var(x) for x in vars_], pm.lc_const(c2))
    return pv, rng, (o.K_EXAMPLE, 0, b"ExampleProofTest", [c2])


def _shuffle_prover(seed, k=4):
    rng = pm.SplitMix64(seed)
    tr = pm.Transcript(b"ShuffleProofTest")
    tr.append_message(b"dom-sep", b"ShuffleProof")
    tr.append_u64(b"k", k)
    pv = pm.Prover(pm.PedersenGens(), tr)
    r = random.Random(seed)
    xs = [r.getrandbits(40) for _ in range(k)]
    ys = list(xs)
    r.shuffle(ys)
    xv = [pv.commit(v, rng.scalar())[1] for v in xs]
    yv = [pv.commit(v, rng.scalar())[1] for v in ys]
    pm.shuffle_gadget(pv, xv, yv)
    return pv, rng, (o.K_SHUFFLE, k, b"ShuffleProofTest", xs + ys)


def _numeric_circuits(gpus):
    def make(provers):
        rp, kd, ix, cf, _ = md.circuit_rows(provers[0].constraints)
        return [g.circuit_create(rp, kd, ix, cf, len(provers[0].a_L), len(provers[0].v)) for g in gpus], None
    return make


def _param_circuits(gpus):
    def make(provers):
        rp, kd, ix, cf, _ = md.circuit_rows(provers[0].constraints, param=True)
        chi = b"".join(md.le(md.circuit_rows(pv.constraints, param=True)[4]) for pv in provers)
        q = len(provers[0].constraints)
        return [g.circuit_create_param(q, 1, rp, kd, ix, cf, len(provers[0].a_L), len(provers[0].v)) for g in gpus], chi
    return make


def _prove_two_party(gpus, builder, seeds, cap, param=False, tamper=None):
    built = [builder(s) for s in seeds]
    provers = [b[0] for b in built]
    m = len(provers[0].v)
    n1 = len(provers[0].a_L)
    # the model's own run of the same circuit (a twin prover: the two-party run consumes its transcript) sizes the phase-2 draws
    twins = [builder(s) for s in seeds]
    models = []
    for (tw, rng, _), s in zip(twins, seeds):
        tr = {}
        models.append((tw.prove(pm.BulletproofGens(cap), rng, tr), tr))
    n2 = len(twins[0][0].a_L) - n1
    blinds = [md.draw_blindings(s, m, n1, n2) for s in seeds]
    dealer = md.Dealer(sum(seeds) + 7)
    gens = _gens(gpus, cap)
    make = _param_circuits(gpus) if param else _numeric_circuits(gpus)
    try:
        proofs, ch, shp = md.run_two_party(gpus, gens, provers, blinds, dealer, make, tamper=tamper)
        return proofs, ch, shp, models, [b[2] for b in built], _V(provers), dealer, gens
    except Exception:
        for g, h in zip(gpus, gens):
            g.gens_destroy(h)
        raise


def _V(provers):
    pc = pm.PedersenGens()
    return [b"".join(pm.p2b(pc.commit(v, vb)) for v, vb in zip(pv.v, pv.v_blinding)) for pv in provers]


def _verify_both(gpus, gens, proofs, ch, shp, meta, V, param, cap):
    """-> (verdicts of the CPU oracle, verdicts of bpgpu_r1cs_verify_batch(_param)) per proof"""
    cpu = [o.r1cs_verify(kind, prm, label, vals[-1:] if kind == o.K_EXAMPLE else [], V[p], md.flat_proof(pr), cap) == 0
           for p, (pr, (kind, prm, label, vals)) in enumerate(zip(proofs, meta))]
    import bp_helpers as bh
    pts = sc = chs = b""
    rr = random.Random(5)
    for p, pr in enumerate(proofs):
        k, pp, ss = bh.verify_inputs(md.flat_proof(pr), V[p])
        pts, sc = pts + pp, sc + ss
        c = ch[p]
        chs += b"".join(md.le(c[key]) for key in ("y", "z", "u", "x", "w")) + md.le(rr.randrange(1, N)) + b"".join(md.le(u) for u in c["us"])
    nb, circ = len(proofs), shp["circuits"][0]
    if param:
        dev = gpus[0].r1cs_verify_batch_param(gens[0], circ, nb, shp["n1"], shp["k"], shp["m"], pts, sc, chs, shp["chi"])[0]
    else:
        dev = gpus[0].r1cs_verify_batch(gens[0], circ, nb, shp["n1"], shp["k"], shp["m"], pts, sc, chs)[0]
    return cpu, [x == 1 for x in dev]


def _cleanup(gpus, gens, shp):
    for g, h, c in zip(gpus, gens, shp["circuits"]):
        g.circuit_destroy(c)
        g.gens_destroy(h)


FIELDS = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6", "t_x", "t_x_blinding", "e_blinding", "L_vec",
          "R_vec", "a", "b")
CASES = {"range8": (_range_prover, 8, False), "example": (_example_prover, 2, False), "shuffle4": (_shuffle_prover, 8, True)}


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("case", sorted(CASES))
def test_two_party_proof_equals_the_model(gpus, case, nb):
    """Two parties' local work on the device opens to Prover.prove's proof (oracle/pymodel.py) field by field: every commitment, T
    point, t_x, t_x_blinding, e_blinding, every L_j, R_j, a and b; the challenges come from the model's transcript fed with the
    opened values.  Every opened quantity passes the MAC check, the parties' modifier planes are identical, and both the CPU oracle
    and bpgpu_r1cs_verify_batch(_param) accept the proofs.  The 4-shuffle is a two-phase circuit proved against ONE parametric
    circuit (second commit call, gadget challenges per proof); the 8-bit range gadget and the example gadget (n = 1) are one-phase."""
    builder, cap, param = CASES[case]
    seeds = [31 + 17 * i for i in range(nb)]
    proofs, ch, shp, models, meta, V, dealer, gens = _prove_two_party(gpus, builder, seeds, cap, param=param)
    try:
        assert dealer.bad == [] and dealer.mod_mismatch == []
        for p, (model, tr) in enumerate(models):
            want = md.model_bytes(model)
            for f in FIELDS:
                assert proofs[p][f] == want[f], (p, f)
            assert [u for u, _ in tr["ipp"]] == ch[p]["us"]
        cpu, dev = _verify_both(gpus, gens, proofs, ch, shp, meta, V, param, cap)
        assert cpu == [True] * nb and dev == [True] * nb
    finally:
        _cleanup(gpus, gens, shp)


@pytest.mark.parametrize("tamper", ["share", "mac", "triple"])
def test_two_party_tampering(gpus, tamper):
    """A party's share of one a_L element changed: the opened proof is rejected by both verifiers.  A MAC share changed: the values
    still open to an accepted proof, but the MAC identity of the commitment that carries it (A_I1) fails.  A triple with z != x y:
    the proof is rejected."""
    proofs, ch, shp, models, meta, V, dealer, gens = _prove_two_party(gpus, _range_prover, [90, 91], 8, tamper=tamper)
    try:
        cpu, dev = _verify_both(gpus, gens, proofs, ch, shp, meta, V, False, 8)
        if tamper == "mac":
            assert cpu == [True, True] and dev == [True, True]
            assert "A_I1[0]" in dealer.bad and "A_O1[0]" not in dealer.bad and "S1[0]" not in dealer.bad
            assert not [x for x in dealer.bad if x.endswith("[1]")]
        else:
            assert cpu == [False, True] and dev == [False, True]
    finally:
        _cleanup(gpus, gens, shp)


def test_two_party_user_sized_range_circuit_equals_single_party_session(gpus):
    """16 x 64-bit range proofs in one circuit (n = 1024) at nb = 1: the opened proof equals, byte for byte, the single-party device
    session (bpgpu_r1cs_prover_commit with explicit s_L / s_R, _session_polys, _ipp_begin, rounds) run with the same blindings and
    challenges; the CPU oracle and bpgpu_r1cs_verify_batch accept it."""
    cap, nvals, seed = 1024, 16, 4242
    r = random.Random(seed)
    vals = [r.getrandbits(64) for _ in range(nvals)]

    def builder(s):
        rng = pm.SplitMix64(s)
        pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"RangeProofTest"))
        for v in vals:
            _, var = pv.commit(v, rng.scalar())
            pm.range_proof_gadget(pv, pm.lc_var(var), v, 64)
        return pv, rng, (o.K_RANGE_MULTI, 64 | (nvals << 16), b"RangeProofTest", vals)

    pv, _, meta = builder(seed)
    m, n = len(pv.v), len(pv.a_L)
    blinds = md.draw_blindings(seed, m, n, 0)
    dealer = md.Dealer(99)
    gens = _gens(gpus, cap)
    proofs, ch, shp = md.run_two_party(gpus, gens, [pv], [blinds], dealer, _numeric_circuits(gpus))
    try:
        assert dealer.mod_mismatch == []
        V = _V([pv])
        cpu, dev = _verify_both(gpus, gens, proofs, ch, shp, [meta], V, False, cap)
        assert cpu == [True] and dev == [True]
        # the single-party session with the same witness, blindings and challenges
        g, c = gpus[0], ch[0]
        pv2 = builder(seed)[0]
        ark = lambda v: b"".join(md.mont(x) for x in v)       # noqa: E731
        ses, com = g.r1cs_prover_commit(gens[0], None, 1, n, ark(pv2.a_L), ark(pv2.a_R), ark(pv2.a_O),
                                        ark([blinds["ib1"], blinds["ob1"], blinds["sb1"]]), s_L=ark(blinds["sL"]), s_R=ark(blinds["sR"]))
        assert com == proofs[0]["A_I1"] + proofs[0]["A_O1"] + proofs[0]["S1"]
        t, _ = g.r1cs_prover_session_polys(ses, shp["circuits"][0], 1, m, md.le(c["y"]), md.le(c["z"]))
        tb = blinds["tb"]
        T = g.msm_gens(gens[0], 5, 0, b"".join(t[32 * j:32 * j + 32] + md.le(b) for j, b in zip((0, 2, 3, 4, 5), tb)))
        assert T == b"".join(proofs[0][f] for f in ("T_1", "T_3", "T_4", "T_5", "T_6"))
        s = g.r1cs_prover_ipp_begin(ses, gens[0], shp["padded"], n, md.le(c["x"]), md.le(c["u"]), None, md.le(c["w"]))
        for j, u in enumerate(c["us"]):
            L, R = g.ipp_round(s, 1)
            assert (L, R) == (proofs[0]["L_vec"][j], proofs[0]["R_vec"][j]), j
            g.ipp_fold(s, md.le(u), md.le(pow(u, -1, N)))
        a, b = g.ipp_finish(s, 1)
        assert (a, b) == (md.le(proofs[0]["a"]), md.le(proofs[0]["b"]))
        g.ipp_destroy(s)
        g.prover_destroy(ses)
    finally:
        _cleanup(gpus, gens, shp)


def test_two_party_refusals(gpus):
    """The single-party calls refuse an authenticated session or IPP, bad shapes give the documented codes, and none of it launches
    anything that changes the session: the proof still opens correctly afterwards (checked by the model test's path)."""
    import ctypes as C
    import mpc_bulletproof_amd as m
    lib, g = m.lib._lib, gpus[0]
    E_ARG, E_LEN = m.lib.E_ARG, m.lib.E_LEN
    gens = _gens([g], 8)[0]
    pv, _, _ = _range_prover(5)
    n, mm = len(pv.a_L), len(pv.v)
    rp, kd, ix, cf, _ = md.circuit_rows(pv.constraints)
    circ = g.circuit_create(rp, kd, ix, cf, n, mm)
    one = md.mont(1) * (3 * n)
    bl = md.mont(1) * 9
    try:
        ses, _ = g.mpc_prover_commit(gens, None, 1, n, one, one, one, one, one, bl)
        h = C.c_void_p()
        out = (C.c_uint8 * 4096)()
        # single-party calls on the authenticated session
        assert lib.bpgpu_r1cs_prover_session_polys(g.ctx, ses, circ, md.le(3), md.le(4), out, out) == E_ARG
        assert lib.bpgpu_r1cs_prover_commit(g.ctx, gens, C.byref(ses), C.c_size_t(3), C.c_size_t(1), one, one, one, one, one, None, bl,
                                            out) == E_ARG
        # vector keys have no place: s_L / s_R missing
        h2 = C.c_void_p()
        assert lib.bpgpu_mpc_prover_commit(g.ctx, gens, C.byref(h2), C.c_size_t(1), C.c_size_t(n), one, one, one, None, None, bl, out) == E_ARG
        assert not h2.value
        # a circuit of another size, out-of-order calls, gadget challenges for a numeric circuit
        rp2, kd2, ix2, cf2, _ = md.circuit_rows(_range_prover(5, 4)[0].constraints)
        c4 = g.circuit_create(rp2, kd2, ix2, cf2, 4, 1)
        trip = md.mont(1) * (54 * n)
        with pytest.raises(m.BpGpuError) as e:
            g.mpc_prover_polys_mask(ses, c4, 1, n, md.le(3), md.le(4), trip)
        assert e.value.code == E_LEN
        g.circuit_destroy(c4)
        with pytest.raises(m.BpGpuError) as e:
            g.mpc_prover_polys_mask(ses, circ, 1, n, md.le(3), md.le(4), trip, gadget_challenges=md.le(5))
        assert e.value.code == E_ARG
        with pytest.raises(m.BpGpuError) as e:
            g.mpc_prover_polys_finish(ses, 1, mm, md.mont(0) * (12 * n), md.mont(1) * 15)
        assert e.value.code == E_ARG
        with pytest.raises(m.BpGpuError) as e:
            g.mpc_prover_ipp_begin(ses, gens, 8, n, md.le(2), md.le(3), md.le(4))
        assert e.value.code == E_ARG
        # non-canonical triple limb
        with pytest.raises(m.BpGpuError) as e:
            g.mpc_prover_polys_mask(ses, circ, 1, n, md.le(3), md.le(4), b"\xff" * 32 + trip[32:])
        assert e.value.code == E_ARG
        g.mpc_prover_polys_mask(ses, circ, 1, n, md.le(3), md.le(4), trip)
        g.mpc_prover_polys_finish(ses, 1, mm, md.mont(0) * (12 * n), md.mont(1) * 15)
        assert lib.bpgpu_r1cs_prover_ipp_begin(g.ctx, ses, gens, C.c_size_t(8), C.c_size_t(n), md.le(2), md.le(3), md.le(5), md.le(4),
                                               C.byref(h)) == E_ARG
        assert lib.bpgpu_r1cs_prover_eval(g.ctx, ses, C.c_size_t(8), md.le(2), out, out) == E_ARG
        ipp = g.mpc_prover_ipp_begin(ses, gens, 8, n, md.le(2), md.le(3), md.le(4))
        # the single-party round and the device-transcript loop refuse shares; a round without its mask is out of order
        assert lib.bpgpu_ipp_round(g.ctx, ipp, out, out) == E_ARG
        assert lib.bpgpu_ipp_run_fs(g.ctx, ipp, bytes(32), out, out, out, out, None) == E_ARG
        assert lib.bpgpu_mpc_ipp_round(g.ctx, ipp, md.mont(0) * 16, out, out) == E_ARG
        # shape errors of the IPP calls
        assert lib.bpgpu_mpc_ipp_mask(g.ctx, ipp, None, out) == E_ARG
        assert lib.bpgpu_mpc_ipp_mask(None, ipp, out, out) == E_ARG
        g.ipp_destroy(ipp)
        g.prover_destroy(ses)
        # a sharded context takes no authenticated session
        g.set_shard(0, 2)
        try:
            h3 = C.c_void_p()
            assert lib.bpgpu_mpc_prover_commit(g.ctx, gens, C.byref(h3), C.c_size_t(1), C.c_size_t(n), one, one, one, one, one, bl, out) == E_ARG
        finally:
            g.set_shard(0, 1)
    finally:
        g.circuit_destroy(circ)
        g.gens_destroy(gens)
