"""Circuits with SEVERAL gadget challenges on the device transcript: labels attached to the circuit handle
(bpgpu_circuit_set_gadget_labels), gadget_label == NULL in every device-transcript entry point -- the verifiers on decoded operands and
on wire bytes, the two-call and the one-call prover, prove-from-values on a context and over a pool, the mixed wire queues -- against
the Python model (tests/multi_challenge_cases.py).  Run with `-m gpu` on an MI355X."""
import pytest

import circuit_gen as cg
import mpc_dealer as md
import multi_challenge_cases as mc
import oracle_lib as o
import prove_fs2_cases as pc

pm = mc.pm
N = mc.N
pytestmark = pytest.mark.gpu
le, cut = md.le, md.cut
IDENT = bytes(64)
SHAPE_IDS = ["n%d+%d-m%d-q%d-chi%d" % s[:5] for s in mc.SHAPES]


@pytest.fixture(scope="module")
def lib():
    import mpc_bulletproof_amd as m
    return m.lib


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gens(gpu):
    g = gpu.gens_create(o.gens("G", mc.CAP), o.gens("H", mc.CAP), o.generator(), o.generator(), 8)
    yield g
    gpu.gens_destroy(g)


def make(gpu, circ, labels="own"):
    """the circuit's handle with its labels attached (labels: another list, or None for none)"""
    h = gpu.circuit_create_param(circ.q, circ.nchi, *circ.csr_param(), circ.n, circ.m)
    if labels is not None:
        gpu.circuit_set_gadget_labels(h, circ.labels if labels == "own" else labels)
    return h


def code_of(lib, call):
    try:
        call()
    except lib.BpGpuError as e:
        return e.code
    return 0


def dims(circ):
    k = mc.lg_padded(circ.n)
    return k, 11 + 2 * k, 1 + 14 * 32 + (2 * k + 2) * 32


def prove(gpu, gens, h, circ, recs, keys):
    """_begin and _finish with gadget_label == NULL -> (commitments, chi, states), (points, scalars, wire, challenges, states)"""
    nb = len(recs)
    sess, com, chi, st = gpu.r1cs_prove_fs2_begin(gens, h, nb, circ.n1, gadget_label=None, nchi=circ.nchi,
                                                  **mc.begin_operands(recs, keys, circ.n1))
    assert sess is not None
    out = gpu.r1cs_prove_fs2_finish(gens, h, sess, nb, circ.n, circ.m, **mc.finish_operands(recs, keys))
    assert not sess.value
    return (com, chi, st), out


_proofs = {}


def proofs_of(gpu, gens, shape, nb):
    """(records, provers the model covers, proof_points, proof_scalars, wire) of a batch: the model's bytes where it proves, the
    device prover's elsewhere (made once)"""
    if (shape, nb) not in _proofs:
        circ = mc.circuit(shape)
        recs, which = mc.batch(shape, nb)
        if len(which) == nb:
            cat = lambda key: b"".join(r[key] for r in recs)      # noqa: E731
            pts, sc, wire = cat("points"), cat("scalars"), cat("wire")
        else:
            h = make(gpu, circ)
            try:
                pts, sc, wire = prove(gpu, gens, h, circ, recs, False)[1][:3]
            finally:
                gpu.circuit_destroy(h)
        _proofs[(shape, nb)] = (recs, which, pts, sc, wire)
    return _proofs[(shape, nb)]


# ------------------------------------------------------------------------------------------------ 1: the verifiers
@pytest.mark.parametrize("nb", mc.BATCHES)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=SHAPE_IDS)
def test_verifiers_accept_draw_the_models_challenges_and_reject_one_tampered_proof(gpu, gens, shape, nb):
    """bpgpu_r1cs_verify_batch_fs2 and _wire2 with attached labels and gadget_label == NULL: every proof accepted, the gadget
    challenges (nb x nchi x 32 B, prover-major) and challenges_out the model verifier's; a flipped bit of t_x in one proof clears its
    bit alone; the labels attached in swapped order reject every proof without an error"""
    circ = mc.circuit(shape)
    k, nvar, plen = dims(circ)
    nchi, n1, m = circ.nchi, circ.n1, circ.m
    recs, which, pts, sc, wire = proofs_of(gpu, gens, shape, nb)
    cat = lambda key: b"".join(r[key] for r in recs)      # noqa: E731
    init, full, com = cat("init"), mc.with_commitments(pts, recs, k), cat("V_compressed")
    for p in which:
        assert recs[p]["accepted"] and pts[64 * nvar * p:64 * nvar * (p + 1)] == recs[p]["points"], p
    h = make(gpu, circ)
    swapped = list(circ.labels)
    swapped[0], swapped[-1] = swapped[-1], swapped[0]
    hs = make(gpu, circ, swapped)
    try:
        ok, _, ch, chi = gpu.r1cs_verify_batch_fs2(gens, h, nb, n1, k, m, nchi, init, None, full, sc)
        assert ok == [1] * nb
        assert len(chi) == 32 * nb * nchi and len(ch) == 32 * nb * (6 + k)
        for p in which:
            assert chi[32 * nchi * p:32 * nchi * (p + 1)] == recs[p]["verifier_chi"], ("gadget challenges", p)
            assert ch[32 * (6 + k) * p:32 * (6 + k) * (p + 1)] == recs[p]["verifier_challenges"], ("challenges", p)
        assert gpu.r1cs_verify_batch_wire2(gens, h, nb, n1, plen, None, wire, com, init) == [1] * nb
        # t_x of the last proof: big-endian on the wire (slot 11 of version 1; its last byte is the low one), little-endian in proof_scalars
        bad = nb - 1
        want = [1] * bad + [0]
        bad_sc, bad_wire = bytearray(sc), bytearray(wire)
        bad_sc[160 * bad] ^= 4
        bad_wire[plen * bad + 1 + 11 * 32 + 31] ^= 4
        ok2, _, ch2, chi2 = gpu.r1cs_verify_batch_fs2(gens, h, nb, n1, k, m, nchi, init, None, full, bytes(bad_sc))
        assert ok2 == want and chi2 == chi
        assert gpu.r1cs_verify_batch_wire2(gens, h, nb, n1, plen, None, bytes(bad_wire), com, init) == want
        assert not mc.verify_model(circ, recs[bad]["p"], recs[bad]["V"], pm.r1cs_proof_from_bytes(bytes(bad_wire[plen * bad:])))[0]
        # the same labels in another order: other challenges, other weights
        ok3, _, _, chi3 = gpu.r1cs_verify_batch_fs2(gens, hs, nb, n1, k, m, nchi, init, None, full, sc)
        assert ok3 == [0] * nb and chi3 != chi
        assert gpu.r1cs_verify_batch_wire2(gens, hs, nb, n1, plen, None, wire, com, init) == [0] * nb
    finally:
        gpu.circuit_destroy(hs)
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ 2: the two-call prover
def check_against_model(first, out, recs, which, circ):
    com, chi, st = first
    k, nvar, plen = dims(circ)
    nchi = circ.nchi
    pts, sc, wire, ch, so = out
    for p in which:
        r = recs[p]
        got = (com[192 * p:192 * (p + 1)], chi[32 * nchi * p:32 * nchi * (p + 1)], st[32 * p:32 * (p + 1)],
               pts[64 * nvar * p:64 * nvar * (p + 1)], sc[160 * p:160 * (p + 1)], wire[plen * p:plen * (p + 1)],
               ch[32 * (5 + k) * p:32 * (5 + k) * (p + 1)], so[32 * p:32 * (p + 1)])
        want = (r["commitments"], r["chi"], r["state_mid"], r["points"], r["scalars"], r["wire"], r["challenges"], r["state_out"])
        for name, g, w in zip(("commitments", "gadget challenges", "state after them", "points", "scalars", "wire", "challenges", "state"),
                              got, want):
            assert g == w, (name, p)


@pytest.mark.parametrize("keys", (False, True), ids=("explicit", "keys"))
@pytest.mark.parametrize("nb", mc.BATCHES)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=SHAPE_IDS)
def test_two_call_proofs_equal_the_model(gpu, gens, shape, nb, keys):
    """commitments, the nchi gadget challenges, the chain after them, proof_points, proof_scalars, wire, challenges_out and states_out
    are the model's bytes, with explicit blinding vectors and with keys"""
    circ = mc.circuit(shape)
    recs, which = mc.batch(shape, nb)
    h = make(gpu, circ)
    try:
        first, out = prove(gpu, gens, h, circ, recs, keys)
    finally:
        gpu.circuit_destroy(h)
    assert len(first[1]) == 32 * nb * circ.nchi and len(out[2]) == nb * dims(circ)[2] and out[2][0] == 1
    check_against_model(first, out, recs, which, circ)


@pytest.mark.parametrize("shape", (mc.SHAPES[0], mc.SHAPES[3]), ids=(SHAPE_IDS[0], SHAPE_IDS[3]))
def test_dev_forms_equal_the_host_forms(gpu, gens, shape):
    """_begin_dev and _finish_dev enqueued back to back on device pointers: the host forms' bytes (65 provers: the session's
    challenges are nb x nchi, the arrays behind them start after all of them)"""
    circ, nb, keys = mc.circuit(shape), 65, True
    recs, _ = mc.batch(shape, nb)
    k, nvar, plen = dims(circ)
    b1, b2 = mc.begin_operands(recs, keys, circ.n1), mc.finish_operands(recs, keys)
    sizes1 = (192 * nb, 32 * nb * circ.nchi, 32 * nb)
    sizes2 = (64 * nb * nvar, 160 * nb, nb * plen, 32 * nb * (5 + k), 32 * nb)
    h = make(gpu, circ)
    bufs = []
    try:
        host1, host2 = prove(gpu, gens, h, circ, recs, keys)
        d1 = {name: gpu.to_device(v) for name, v in b1.items() if v is not None}
        d2 = {name: gpu.to_device(v) for name, v in b2.items() if v is not None}
        o1, o2 = [gpu.malloc(s) for s in sizes1], [gpu.malloc(s) for s in sizes2]
        bufs = list(d1.values()) + list(d2.values()) + o1 + o2
        sess = gpu.r1cs_prove_fs2_begin_dev(gens, h, nb, circ.n1, d1["states"], None, d1["blindings"], d_a_L=d1.get("a_L"),
                                            d_a_R=d1.get("a_R"), d_a_O=d1.get("a_O"), d_vector_keys=d1.get("vector_keys"),
                                            d_commitments=o1[0], d_chi=o1[1], d_states_out=o1[2])
        gpu.r1cs_prove_fs2_finish_dev(gens, h, sess, d2["a_L"], d2["a_R"], d2["a_O"], d2["blindings"], o2[0], o2[1],
                                      d_v_blinding=d2.get("v_blinding"), d_vector_keys=d2["vector_keys"], d_wire=o2[2], d_ch=o2[3],
                                      d_states_out=o2[4])
        assert not sess.value and gpu.input_flag() == 0
        assert tuple(gpu.download(p, s) for p, s in zip(o1, sizes1)) == host1
        assert tuple(gpu.download(p, s) for p, s in zip(o2, sizes2)) == host2
    finally:
        for b in bufs:
            gpu.free(b)
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ 3, 4: a gate program with two challenges
@pytest.fixture(scope="module")
def shuffles(gpu):
    """the two-shuffle program, its circuit with both labels attached, and three provers"""
    prog, outs = mc.two_shuffles_program()
    rows = mc.two_shuffles_rows(prog, outs)
    rp, kd, ix, cf, _ = md.circuit_rows(rows, nchi=2)
    circ = gpu.circuit_create_param(len(rows), 2, rp, kd, ix, cf, prog.n, prog.m)
    gpu.circuit_set_gadget_labels(circ, mc.SHUFFLE_LABELS)
    w = gpu.witness_create(*prog.create_args())
    yield dict(prog=prog, csr=(len(rows), 2, rp, kd, ix, cf), circ=circ, w=w, provers=[mc.two_shuffles_prover(p) for p in range(3)])
    gpu.witness_destroy(w)
    gpu.circuit_destroy(circ)


def one_call_operands(recs, keys, states="state_in"):
    cat = lambda key: b"".join(r[key] for r in recs)      # noqa: E731
    kw = dict(v=cat("v"), v_blinding=cat("v_blinding"), blindings=cat("blindings"))
    kw["states" if states == "state_in" else "init_states"] = cat(states)
    kw.update(dict(vector_keys=cat("keys")) if keys else dict(s_L=cat("s_L"), s_R=cat("s_R")))
    return kw


_one_call = {}


def one_call(gpu, gens, shuffles, nb):
    """bpgpu_r1cs_prove_fs2 on the first nb provers (keys; default options), once"""
    if nb not in _one_call:
        prog = shuffles["prog"]
        _one_call[nb] = gpu.r1cs_prove_fs2(gens, shuffles["circ"], shuffles["w"], nb, prog.n, prog.m, gadget_label=None, nchi=2,
                                           want_witness=True, **one_call_operands(shuffles["provers"][:nb], True))
    return _one_call[nb]


@pytest.mark.parametrize("nb", (1, 3))
def test_one_call_prover_equals_the_two_calls_on_the_host_witness(gpu, gens, shuffles, nb):
    """bpgpu_r1cs_prove_fs2 on the two-shuffle program: the first chain is evaluated on chi_1, the second on chi_2 (the planes are
    the host evaluator's on the challenges returned); the proof bytes are those of _begin / _finish fed that witness, with keys and
    with explicit vectors, with BPGPU_OPT_WITNESS_SCAN_MIN 0 and 1; bpgpu_r1cs_verify_batch_wire2 accepts them"""
    prog, circ, w = shuffles["prog"], shuffles["circ"], shuffles["w"]
    recs = shuffles["provers"][:nb]
    n, m = prog.n, prog.m
    k = mc.lg_padded(n)
    plen = 1 + 14 * 32 + (2 * k + 2) * 32
    cat = lambda key: b"".join(r[key] for r in recs)      # noqa: E731
    pts, sc, wire, ch, so, chi, planes = one_call(gpu, gens, shuffles, nb)
    assert len(chi) == 64 * nb and len(wire) == nb * plen
    want = [[], [], []]
    for p, r in enumerate(recs):
        c = tuple(int.from_bytes(chi[64 * p + 32 * j:64 * p + 32 * j + 32], "little") for j in range(2))
        assert c[0] != c[1]
        for plane, vals in zip(want, prog.evaluate(r["v_int"], (), c)):
            plane.append(mc.ark(vals))
    want = tuple(b"".join(x) for x in want)
    assert planes == want
    old = gpu.get_option("witness_scan_min")
    try:
        for scan_min in (0, 1):
            gpu.set_option("witness_scan_min", scan_min)
            for keys in (True, False):
                got = gpu.r1cs_prove_fs2(gens, circ, w, nb, n, m, gadget_label=None, nchi=2, want_witness=True, **one_call_operands(recs, keys))
                assert got == (pts, sc, wire, ch, so, chi, planes), (scan_min, keys)
    finally:
        gpu.set_option("witness_scan_min", old)
    sess, _, chi2, _ = gpu.r1cs_prove_fs2_begin(gens, circ, nb, 0, gadget_label=None, nchi=2, states=cat("state_in"), blindings=cat("bl1"))
    assert chi2 == chi
    two = gpu.r1cs_prove_fs2_finish(gens, circ, sess, nb, n, m, a_L=want[0], a_R=want[1], a_O=want[2], blindings=cat("bl2"),
                                    v_blinding=cat("v_blinding"), vector_keys=cat("key2"))
    assert two == (pts, sc, wire, ch, so)
    assert gpu.r1cs_verify_batch_wire2(gens, circ, nb, 0, plen, None, wire, cat("V_compressed"), cat("init")) == [1] * nb


def check_prove_values(got, ref, provers, prog):
    """prover 1 (a wrong value) rejected with zero proof rows and its diagnostics intact, the others' bytes those of the one call"""
    nb, n = 3, prog.n
    k = mc.lg_padded(n)
    nvar, plen = 11 + 2 * k, 1 + 14 * 32 + (2 * k + 2) * 32
    pts, sc, wire, ch, so, chi, planes = ref
    assert got.ok == [1, 0, 1]
    assert got.first_bad_row[0] == got.first_bad_row[2] == -1 and got.first_bad_row[1] == 2 * n + 1      # the second shuffle's equality
    assert got.V == b"".join(r["V_xy"] for r in provers) and got.V_compressed == b"".join(r["V_compressed"] for r in provers)
    for name, g, w, size in (("points", got.points, pts, 64 * nvar), ("scalars", got.scalars, sc, 160), ("wire", got.wire, wire, plen),
                             ("challenges", got.challenges, ch, 32 * (5 + k)), ("states", got.states, so, 32)):
        assert g[size:2 * size] == bytes(size), name
        assert g[:size] == w[:size] and g[2 * size:] == w[2 * size:], name
    # the diagnostics: the challenges and the witness of the rejected prover stay
    assert len(got.chi) == 64 * nb and got.chi[:64] == chi[:64] and got.chi[128:] == chi[128:] and got.chi[64:128] != bytes(64)
    c = tuple(int.from_bytes(got.chi[64 + 32 * j:96 + 32 * j], "little") for j in range(2))
    for plane, ref_plane, vals in zip(got.planes, planes, prog.evaluate(provers[1]["v_int"], (), c)):
        assert plane[32 * n:64 * n] == mc.ark(vals)
        assert plane[:32 * n] == ref_plane[:32 * n] and plane[64 * n:] == ref_plane[64 * n:]


def test_prove_values_on_a_context_and_over_a_pool(gpu, gens, shuffles):
    """bpgpu_r1cs_prove_values and bpgpu_pool_r1cs_prove_values (two slots of device 0) on three provers, prover 1 with y_2 no
    permutation of x_2"""
    import mpc_bulletproof_amd as mm
    prog = shuffles["prog"]
    n, m = prog.n, prog.m
    ref = one_call(gpu, gens, shuffles, 3)
    provers = [shuffles["provers"][0], mc.two_shuffles_prover(1, wrong=True), shuffles["provers"][2]]
    ops = one_call_operands(provers, True, states="init")
    got = gpu.r1cs_prove_values(gens, shuffles["circ"], shuffles["w"], 3, n, m, gadget_label=None, nchi=2, want_witness=True, **ops)
    check_prove_values(got, ref, provers, prog)
    pool = mm.BpPool((0, 0))
    pg = pc_ = pw = None
    try:
        pg = pool.gens_create(o.gens("G", mc.CAP), o.gens("H", mc.CAP), o.generator(), o.generator(), 8)
        pc_ = pool.circuit_create_param(*shuffles["csr"], n, m)
        pool.circuit_set_gadget_labels(pc_, mc.SHUFFLE_LABELS)
        pw = pool.witness_create(*prog.create_args())
        got = pool.r1cs_prove_values(pg, pc_, pw, 3, n, m, gadget_label=None, nchi=2, want_witness=True, **ops)
        check_prove_values(got, ref, provers, prog)
    finally:
        if pw is not None:
            pool.witness_destroy(pw)
        if pc_ is not None:
            pool.circuit_destroy(pc_)
        if pg is not None:
            pool.gens_destroy(pg)
        pool.close()


# ------------------------------------------------------------------------------------------------ 5: mixed wire queues
def test_mixed_wire_queue_of_three_kinds_of_circuit(gpu, gens):
    """a one-phase circuit (1 proof), a circuit with one challenge under the group's gadget_label (65 proofs) and a circuit with
    three challenges under attached labels (3 proofs, the last one tampered) in one queue: the screened verdicts are the model's
    (for the 65: of proofs 0, 63 and 64; the others are honest provers' proofs), the combined point is the identity exactly without
    the tampered proof"""
    import random
    rnd = random.Random(515)
    rho = lambda nb: b"".join(le(rnd.randrange(1, N)) for _ in range(nb))      # noqa: E731
    # a: one phase
    ca = cg.Circuit(71, 2, 0, 1, 3, 0, "sparse")
    proof_a, info_a = cg.prove(ca, mc.mgens())
    ka = mc.lg_padded(ca.n)
    wire_a = pm.r1cs_proof_to_bytes(proof_a)
    assert cg.verifier(ca, info_a["V"])[0].verify(proof_a, mc.mgens()) and len(wire_a) == 1 + 11 * 32 + (2 * ka + 2) * 32
    # b: one challenge, the label with the group
    shape_b = pc.SHAPES[2]
    cb = pc.circuit(shape_b)
    rb = {p: pc.model_proof(cb, mc.mgens(), p, (False, False), 700 + shape_b[0]) for p in (0, 63, 64)}
    recs_b = []
    for p in range(65):
        recs_b.append(rb[p] if p in rb else dict(rb[0], state_in=mc.state_after_commitments(p, rb[0]["V"])))
    kb = mc.lg_padded(cb.n)
    plen_b = 1 + 14 * 32 + (2 * kb + 2) * 32
    # c: three challenges, the labels with the circuit
    shape_c = mc.SHAPES[2]
    cc = mc.circuit(shape_c)
    recs_c = [mc.record(shape_c, p) for p in range(3)]
    _, _, plen_c = dims(cc)
    wire_c = bytearray(b"".join(r["wire"] for r in recs_c))
    good_c = bytes(wire_c)
    wire_c[2 * plen_c + 1 + 11 * 32 + 31] ^= 1
    want_c = [int(mc.verify_model(cc, p, recs_c[p]["V"], pm.r1cs_proof_from_bytes(bytes(wire_c[plen_c * p:plen_c * (p + 1)])))[0])
              for p in range(3)]
    assert want_c == [1, 1, 0]
    ha = gpu.circuit_create(*ca.csr(), ca.n, ca.m)
    hb = gpu.circuit_create_param(cb.q, 1, *cb.csr_param(), cb.n, cb.m)
    hc = make(gpu, cc)
    try:
        sess, _, _, _ = gpu.r1cs_prove_fs2_begin(gens, hb, 65, cb.n1, gadget_label=cg.CHI_LABEL, **pc.begin_operands(recs_b, (False, False), cb.n1))
        wire_b = gpu.r1cs_prove_fs2_finish(gens, hb, sess, 65, cb.n, cb.m, **pc.finish_operands(recs_b, (False, False)))[2]
        for p in rb:
            assert wire_b[plen_b * p:plen_b * (p + 1)] == rb[p]["wire"], p
            vf = pm.Verifier(pm.PedersenGens(), pm.Transcript(mc.label(p)))
            cb.install(vf, commitments=rb[p]["V"])
            assert vf.verify(rb[p]["proof"], mc.mgens()), p

        def groups(wc_bytes):
            return [
                dict(circuit=ha, nb=1, n1=ca.n, proof_len=len(wire_a), proofs=wire_a,
                     commitments=b"".join(pm.point_compress(v) for v in info_a["V"]), init_states=pm.Transcript(cg.LABEL).state,
                     gadget_label=None, rho=rho(1)),
                dict(circuit=hb, nb=65, n1=cb.n1, proof_len=plen_b, proofs=wire_b,
                     commitments=b"".join(pm.point_compress(v) for r in recs_b for v in r["V"]),
                     init_states=b"".join(pm.Transcript(mc.label(p)).state for p in range(65)), gadget_label=cg.CHI_LABEL, rho=rho(65)),
                dict(circuit=hc, nb=3, n1=cc.n1, proof_len=plen_c, proofs=bytes(wc_bytes),
                     commitments=b"".join(r["V_compressed"] for r in recs_c), init_states=b"".join(r["init"] for r in recs_c),
                     gadget_label=None, rho=rho(3))]
        oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, groups(good_c))
        assert oks == [[1], [1] * 65, [1, 1, 1]] and nf == 0
        assert gpu.r1cs_verify_mixed_wire_combined(gens, groups(good_c)) == IDENT
        oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, groups(wire_c))
        assert oks == [[1], [1] * 65, want_c] and nf == 1
        assert gpu.r1cs_verify_mixed_wire_combined(gens, groups(wire_c)) != IDENT
    finally:
        for h in (ha, hb, hc):
            gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ 6: one challenge, the label attached
def test_one_challenge_with_an_attached_label_gives_the_bytes_of_the_label_passed(gpu, gens):
    shape = pc.SHAPES[3]
    circ = pc.circuit(shape)
    nb = 2
    recs = [pc.model_proof(circ, mc.mgens(), p, (False, True), 700 + shape[0]) for p in range(nb)]
    k = mc.lg_padded(circ.n)
    plen = 1 + 14 * 32 + (2 * k + 2) * 32
    vk = (False, True)
    h_arg = gpu.circuit_create_param(circ.q, 1, *circ.csr_param(), circ.n, circ.m)
    h_own = gpu.circuit_create_param(circ.q, 1, *circ.csr_param(), circ.n, circ.m)
    gpu.circuit_set_gadget_labels(h_own, [b"another label"])
    gpu.circuit_set_gadget_labels(h_own, [cg.CHI_LABEL])          # a second call replaces the labels
    try:
        out = {}
        for name, h, lab in (("passed", h_arg, cg.CHI_LABEL), ("attached", h_own, None)):
            sess, com, chi, st = gpu.r1cs_prove_fs2_begin(gens, h, nb, circ.n1, gadget_label=lab, **pc.begin_operands(recs, vk, circ.n1))
            fin = gpu.r1cs_prove_fs2_finish(gens, h, sess, nb, circ.n, circ.m, **pc.finish_operands(recs, vk))
            pts, sc, wire = fin[:3]
            full = b"".join(pts[64 * (11 + 2 * k) * p:][:6 * 64] + b"".join(pm.p2b(v) for v in recs[p]["V"]) +
                            pts[64 * (11 + 2 * k) * p:][6 * 64:64 * (11 + 2 * k)] for p in range(nb))
            init = b"".join(pm.Transcript(mc.label(p)).state for p in range(nb))
            cmp_ = b"".join(pm.point_compress(v) for p in range(nb) for v in recs[p]["V"])
            ver = gpu.r1cs_verify_batch_fs2(gens, h, nb, circ.n1, k, circ.m, 1, init, lab, full, sc)
            out[name] = (com, chi, st, fin, ver, gpu.r1cs_verify_batch_wire2(gens, h, nb, circ.n1, plen, lab, wire, cmp_, init))
        assert out["attached"] == out["passed"]
        assert out["passed"][3][2] == b"".join(r["wire"] for r in recs) and out["passed"][4][0] == [1] * nb and out["passed"][5] == [1] * nb
    finally:
        gpu.circuit_destroy(h_own)
        gpu.circuit_destroy(h_arg)


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals(gpu, gens, lib, shuffles):
    E = lib.E_ARG
    shape = mc.SHAPES[1]
    circ = mc.circuit(shape)
    k, nvar, plen = dims(circ)
    recs, _ = mc.batch(shape, 1)
    r = recs[0]
    full = mc.with_commitments(r["points"], recs, k)
    numeric = cg.Circuit(7, 2, 0, 1, 3, 0, "sparse")
    h = make(gpu, circ)
    bare = make(gpu, circ, None)
    hn = gpu.circuit_create(*numeric.csr(), numeric.n, numeric.m)
    prog3 = mc.wc.Program(shuffles["prog"].m, nchi=3)
    prog3.end_phase1()
    for _ in range(shuffles["prog"].n):
        prog3.mul([(mc.wc.V, 0, 1)], [(mc.wc.V, 1, 1)])
    w3 = gpu.witness_create(*prog3.create_args())
    lab = circ.labels[0]
    b1, b2 = mc.begin_operands(recs, False, circ.n1), mc.finish_operands(recs, False)
    group = dict(circuit=h, nb=1, n1=circ.n1, proof_len=plen, proofs=r["wire"], commitments=r["V_compressed"], init_states=r["init"],
                 rho=le(5))
    sp, sprog = shuffles["provers"][:1], shuffles["prog"]
    try:
        # set_gadget_labels itself
        assert code_of(lib, lambda: gpu.circuit_set_gadget_labels(hn, [lab])) == E          # a numeric circuit
        assert code_of(lib, lambda: gpu.circuit_set_gadget_labels(bare, None)) == E        # null labels
        # attached labels and a label with the call
        calls_with_label = [
            lambda x: gpu.r1cs_verify_batch_fs2(gens, x, 1, circ.n1, k, circ.m, circ.nchi, r["init"], lab, full, r["scalars"]),
            lambda x: gpu.r1cs_verify_batch_wire2(gens, x, 1, circ.n1, plen, lab, r["wire"], r["V_compressed"], r["init"]),
            lambda x: gpu.r1cs_prove_fs2_begin(gens, x, 1, circ.n1, gadget_label=lab, nchi=circ.nchi, **b1),
            lambda x: gpu.r1cs_verify_mixed_wire_screened(gens, [dict(group, circuit=x, gadget_label=lab)]),
            lambda x: gpu.r1cs_verify_mixed_wire_combined(gens, [dict(group, circuit=x, gadget_label=lab)])]
        for i, call in enumerate(calls_with_label):
            assert code_of(lib, lambda: call(h)) == E, i
            assert code_of(lib, lambda: call(bare)) == E, i          # nothing attached: two challenges stay refused, label or not
        # nothing attached and no label
        calls_without = [
            lambda x: gpu.r1cs_verify_batch_fs2(gens, x, 1, circ.n1, k, circ.m, circ.nchi, r["init"], None, full, r["scalars"]),
            lambda x: gpu.r1cs_verify_batch_wire2(gens, x, 1, circ.n1, plen, None, r["wire"], r["V_compressed"], r["init"]),
            lambda x: gpu.r1cs_prove_fs2_begin(gens, x, 1, circ.n1, gadget_label=None, nchi=circ.nchi, **b1),
            lambda x: gpu.r1cs_verify_mixed_wire_screened(gens, [dict(group, circuit=x, gadget_label=None)])]
        for i, call in enumerate(calls_without):
            assert code_of(lib, lambda: call(bare)) == E, i
        # ... also where one challenge would do: the label is missing
        one = pc.circuit(pc.SHAPES[2])
        h1 = gpu.circuit_create_param(one.q, 1, *one.csr_param(), one.n, one.m)
        try:
            plen1 = 1 + 14 * 32 + (2 * 1 + 2) * 32
            assert code_of(lib, lambda: gpu.r1cs_verify_batch_wire2(gens, h1, 1, one.n1, plen1, None, bytes(plen1), bytes(32), bytes(32))) == E
            assert code_of(lib, lambda: gpu.r1cs_prove_fs2_begin(gens, h1, 1, one.n1, gadget_label=None, **b1)) == E
            assert code_of(lib, lambda: gpu.r1cs_verify_mixed_wire_screened(
                gens, [dict(group, circuit=h1, proof_len=plen1, proofs=bytes(plen1), gadget_label=None)])) == E
        finally:
            gpu.circuit_destroy(h1)
        # the one-call provers: a label beside the attached ones, and a program whose nchi is not the circuit's
        ops = one_call_operands(sp, True)
        opv = one_call_operands(sp, True, states="init")
        n, m = sprog.n, sprog.m
        assert code_of(lib, lambda: gpu.r1cs_prove_fs2(gens, shuffles["circ"], shuffles["w"], 1, n, m, gadget_label=lab, nchi=2, **ops)) == E
        assert code_of(lib, lambda: gpu.r1cs_prove_values(gens, shuffles["circ"], shuffles["w"], 1, n, m, gadget_label=lab, nchi=2, **opv)) == E
        assert code_of(lib, lambda: gpu.r1cs_prove_fs2(gens, shuffles["circ"], w3, 1, n, m, gadget_label=None, nchi=2, **ops)) == E
        assert code_of(lib, lambda: gpu.r1cs_prove_values(gens, shuffles["circ"], w3, 1, n, m, gadget_label=None, nchi=2, **opv)) == E
        # ... and after all these refusals the handle still proves and verifies
        first, out = prove(gpu, gens, h, circ, recs, False)
        check_against_model(first, out, recs, (0,), circ)
        assert b2 and gpu.r1cs_verify_batch_wire2(gens, h, 1, circ.n1, plen, None, r["wire"], r["V_compressed"], r["init"]) == [1]
    finally:
        gpu.witness_destroy(w3)
        for x in (h, bare, hn):
            gpu.circuit_destroy(x)
