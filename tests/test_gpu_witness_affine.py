"""The affine instantiation of the scan form (csrc/k_witness.hip k_witness_scan<true>: extended chains as a segmented prefix composition
of affine maps) on the GPU against Program.evaluate on Python integers, byte for byte on every gate of every prover: the programs of
tests/witness_affine_cases.py with BPGPU_OPT_WITNESS_SCAN_MIN = 1 and = 0 and on the forced routes; device buffers; the phases one
after the other; the constraint check on a 300-Horner gadget; and the one-call two-phase prover with its Horner gadget scanned."""
import random

import pytest

import witness_cases as wc
import witness_chain_cases as cc
import witness_affine_cases as ac
from test_gpu_witness_scan import default_scan_min, scanned

pytestmark = pytest.mark.gpu
pm = wc.pm
N = wc.N
NBS = (1, 3, 65)
NAMES = [c.name for c in ac.cases()]
LONG = "afflong2x%d" % ac.LONG


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def program(gpu):
    """name -> the case's resident program (created once)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = gpu.witness_create(*ac.case(name).prog.create_args())
        return made[name]
    yield get
    for w in made.values():
        gpu.witness_destroy(w)


_rows = {}


def planes(case, nb):
    """the expected planes of a batch, ark form (a prover's rows encoded once, however often the batch repeats it)"""
    for p in range(min(nb, len(case.provers))):
        if (case.name, p) not in _rows:
            _rows[(case.name, p)] = tuple(b"".join(wc.mont(x) for x in plane) for plane in case.want(p))
    return tuple(b"".join(_rows[(case.name, p % len(case.provers))][k] for p in range(nb)) for k in range(3))


@pytest.fixture(autouse=True)
def restore(gpu):
    yield
    scanned(gpu, default_scan_min())


@pytest.mark.parametrize("name", NAMES)
def test_affine_scan_equals_the_model_on_every_route(gpu, program, name):
    case, w = ac.case(name), program(name)
    n = case.prog.n
    for nb in (NBS[:2] if name == LONG else NBS):
        v, inputs, chi = case.operands(nb)
        want = planes(case, nb)
        for scan_min in (1, 0):
            scanned(gpu, scan_min)
            assert gpu.r1cs_witness_synthesize(w, nb, n, 0, v, inputs, chi) == want, (nb, scan_min)
        for route in (1, 2):                                             # the forced routes, whatever the option says
            gpu.set_option("witness_scan_min", 1)
            gpu.set_option("witness_route", route)
            assert gpu.r1cs_witness_synthesize(w, nb, n, 0, v, inputs, chi) == want, (nb, route)
    # ... and on device buffers that held something else
    nb = 3
    v, inputs, chi = case.operands(nb)
    bufs = [gpu.to_device(x) if x else None for x in (v, inputs, chi)] + [gpu.to_device(wc.mont(12345) * (nb * n)) for _ in range(3)]
    try:
        scanned(gpu, 1)
        gpu.r1cs_witness_synthesize_dev(w, nb, 0, *bufs[3:], d_v=bufs[0], d_inputs=bufs[1], d_gadget_challenges=bufs[2])
        assert tuple(gpu.download(p, 32 * nb * n) for p in bufs[3:]) == planes(case, nb)
        assert gpu.input_flag() == 0
    finally:
        for p in bufs:
            if p:
                gpu.free(p)


def test_gen70dense_with_its_two_affine_members_scanned(gpu):
    """the one earlier program that gains affine members (two chains of one): scanned and not, the same bytes"""
    case = wc.case("gen70dense")
    assert ac.figures(case.prog)["affine1"] == ac.figures(case.prog)["affine2"] == 1
    w = gpu.witness_create(*case.prog.create_args())
    try:
        v, inputs, chi = case.operands(3)
        want = case.planes(3)
        for scan_min in (1, 0):
            scanned(gpu, scan_min)
            assert gpu.r1cs_witness_synthesize(w, 3, case.prog.n, 0, v, inputs, chi) == want, scan_min
    finally:
        gpu.witness_destroy(w)


def test_phase_one_then_phase_two_equals_phase_zero(gpu, program):
    case, w = ac.case("affmixed"), program("affmixed")
    n, n1, nb = case.prog.n, case.prog.phase1, 3
    v, inputs, chi = case.operands(nb)
    want = planes(case, nb)
    marker = wc.mont(12345)
    scanned(gpu, 1)
    held = tuple(marker * (nb * n) for _ in range(3))
    first = gpu.r1cs_witness_synthesize(w, nb, n, 1, v, inputs, None, *held)
    for plane, full in zip(first, want):
        for p in range(nb):
            row = plane[32 * n * p:32 * n * (p + 1)]
            assert row[:32 * n1] == full[32 * n * p:32 * (n * p + n1)] and row[32 * n1:] == marker * (n - n1), p
    assert gpu.r1cs_witness_synthesize(w, nb, n, 2, v, inputs, chi, *first) == want
    assert gpu.r1cs_witness_synthesize(w, nb, n, 0, v, inputs, chi) == want


def _constraints(case, p):
    """(the model's constraints after the gadget ran on prover p, how many of them are phase 1's)"""
    return case.model(p).constraints, len(wc.pm_constraints_phase1(case, p))


def test_scanned_horner_satisfies_its_circuit_and_a_broken_one_does_not(gpu, program):
    case, w = ac.case("horner300"), program("horner300")
    prog = case.prog
    assert ac.figures(prog)["longest2"] == 298 and cc.figures(prog)["longest2"] == 0
    nb = 2
    q, nchi, rp, kd, ix, cf = ac.horner_circuit(*_constraints(case, 3))
    circ = gpu.circuit_create_param(q, nchi, rp, kd, ix, cf, prog.n, prog.m)

    def broken(p):
        v, inputs, chi = case.prover(p + 3)
        v2, inputs2 = case.breaker(v, inputs)
        return v2, inputs2, chi
    try:
        for which, verdict in ((lambda p: case.prover(p + 3), [1, 1]), (broken, [0, 0])):       # provers 3, 4: random challenges
            v, inputs, chi = case.operands(nb, which)
            scanned(gpu, 1)
            got = gpu.r1cs_witness_synthesize(w, nb, prog.n, 0, v, inputs, chi)
            scanned(gpu, 0)
            assert got == gpu.r1cs_witness_synthesize(w, nb, prog.n, 0, v, inputs, chi)
            if verdict[0]:
                assert got == tuple(b"".join(wc.mont(x) for p in range(nb) for x in case.want(p + 3)[k]) for k in range(3))
            ok, row, gate, _ = gpu.r1cs_constraints_satisfied(circ, nb, q, *got, v=v, gadget_challenges=chi)
            assert ok == verdict and gate == [-1] * nb                                          # (the gates hold either way)
    finally:
        gpu.circuit_destroy(circ)


def _record(one, mgens, case, p):
    """test_gpu_prove_fs2_onecall.record for a case handed in (that one looks its case up by name): the operands of the call for prover
    p and the model's outputs, under the transcript's own gadget challenge"""
    from prove_fs_cases import Replay, label
    le, ark = one.le, one.ark
    prog = case.prog
    n, n1 = prog.n, prog.phase1
    v, inputs, _ = case.prover(p)
    rnd = random.Random(19000 + 10 * p)
    vb = [rnd.randrange(N) for _ in range(prog.m)]
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(label(p)))
    committed = [pv.commit(x, b) for x, b in zip(v, vb)]
    case.gadget(pv, [c[1] for c in committed], v, inputs)
    q1, state_in = len(pv.constraints), pv.transcript.state
    drawn = []
    draw = pv.challenge_scalar
    pv.challenge_scalar = lambda lab: drawn.append(draw(lab)) or drawn[-1]
    bl1 = [rnd.randrange(N) for _ in range(3)]
    key1, key2 = (bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(2))
    bl2 = [rnd.randrange(N) for _ in range(3)]
    tb = [rnd.randrange(N) for _ in range(5)]
    (sL1, sR1), (sL2, sR2) = one._expand(key1, n1), one._expand(key2, n - n1)
    trace = {}
    rng = Replay(bl1 + sL1 + sR1 + bl2 + sL2 + sR2 + tb)
    proof = pv.prove(mgens, rng, trace=trace)
    assert not rng.values and len(drawn) == 1 and len(pv.a_L) == n
    assert tuple(prog.evaluate(v, inputs, (drawn[0],))) == (pv.a_L, pv.a_R, pv.a_O)           # the program is the gadget
    order = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6")
    points = b"".join(pm.p2b(proof[k]) for k in order) + b"".join(map(pm.p2b, proof["L_vec"])) + b"".join(map(pm.p2b, proof["R_vec"]))
    return dict(
        state_in=state_in, v=ark(v), inputs=b"", v_blinding=ark(vb), blindings=ark(bl1 + bl2 + tb), keys=key1 + key2, bl1=ark(bl1),
        bl2=ark(bl2 + tb), key1=key1, key2=key2, planes=tuple(ark(x) for x in (pv.a_L, pv.a_R, pv.a_O)), chi=le(drawn[0]),
        constraints=pv.constraints, q1=q1, V=b"".join(pm.point_compress(c[0]) for c in committed), init=pm.Transcript(label(p)).state,
        points=points, scalars=b"".join(le(proof[k]) for k in ("t_x", "t_x_blinding", "e_blinding", "a", "b")),
        challenges=b"".join(le(trace[k]) for k in "yzuxw") + b"".join(le(u) for u, _ in trace["ipp"]),
        state_out=pv.transcript.state, wire=pm.r1cs_proof_to_bytes(proof))


def test_one_call_prover_with_the_horner_gadget_scanned(gpu):
    """bpgpu_r1cs_prove_fs2 on horner_case(9) with scan_min = 1: the model's bytes, the bytes of _begin / _finish fed the
    Python-evaluated witness, and a wire that bpgpu_r1cs_verify_batch_wire2 accepts"""
    import oracle_lib as o
    import test_gpu_prove_fs2_onecall as one
    from prove_fs_cases import lg_padded
    gens = gpu.gens_create(o.gens("G", one.CAP), o.gens("H", one.CAP), o.generator(), o.generator(), 8)
    case = ac.horner_case(9)
    n, m, n1 = case.prog.n, case.prog.m, case.prog.phase1
    nb, keys = 2, True
    mgens = one.ModelGens(one.CAP)
    recs = [_record(one, mgens, case, p) for p in range(nb)]
    cat = lambda key: b"".join(r[key] for r in recs)      # noqa: E731
    plen = 1 + 14 * 32 + (2 * lg_padded(n) + 2) * 32
    q, nchi, rp, kd, ix, cf = ac.horner_circuit(recs[0]["constraints"], recs[0]["q1"])
    circ, w = gpu.circuit_create_param(q, 1, rp, kd, ix, cf, n, m), gpu.witness_create(*case.prog.create_args())
    try:
        scanned(gpu, 1)
        pts, sc, wire, ch, so, chi, got = gpu.r1cs_prove_fs2(gens, circ, w, nb, n, m, gadget_label=one.LABEL, want_witness=True,
                                                             **one.operands(recs, keys))
        assert chi == cat("chi") and got == tuple(b"".join(r["planes"][i] for r in recs) for i in range(3))
        scanned(gpu, 0)
        assert one.two_calls(gpu, gens, circ, case, recs, keys) == (pts, sc, wire, ch, so)
        assert (pts, sc, wire, ch, so) == (cat("points"), cat("scalars"), cat("wire"), cat("challenges"), cat("state_out"))
        assert gpu.r1cs_verify_batch_wire2(gens, circ, nb, n1, plen, one.LABEL, wire, cat("V"), cat("init")) == [1] * nb
    finally:
        gpu.witness_destroy(w)
        gpu.circuit_destroy(circ)
        gpu.gens_destroy(gens)
