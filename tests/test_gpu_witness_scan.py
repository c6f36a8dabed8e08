"""The scan form of the witness synthesis (csrc/k_witness.hip k_witness_scan: product chains as a segmented prefix product) on the GPU
against Program.evaluate on Python integers, byte for byte on every gate of every prover: the chain programs of
tests/witness_chain_cases.py and the reference's chain gadgets with BPGPU_OPT_WITNESS_SCAN_MIN = 1 and = 0; the phases one after the
other; the constraint check on a 300-shuffle; the option itself; and the one-call two-phase prover with its gadget scanned."""
import re
import os

import pytest

import witness_cases as wc
import witness_chain_cases as cc

pytestmark = pytest.mark.gpu
N = wc.N
NBS = (1, 3, 65)
NEW = [c.name for c in cc.cases()]
GADGETS = ("shuffle2", "shuffle3", "shuffle4", "shuffle9", "composite")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def find(name):
    return cc.case(name) if name in NEW else (cc.shuffle(300) if name == "shuffle300" else wc.case(name))


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
            made[name] = gpu.witness_create(*find(name).prog.create_args())
        return made[name]
    yield get
    for w in made.values():
        gpu.witness_destroy(w)


_rows = {}


def planes(case, nb, lo=0, hi=None):
    """the expected planes of a batch, ark form (a prover's rows encoded once, however often the batch repeats it)"""
    hi = case.prog.n if hi is None else hi
    for p in range(min(nb, len(case.provers))):
        if (case.name, p) not in _rows:
            _rows[(case.name, p)] = tuple([wc.mont(x) for x in plane] for plane in case.want(p))
    return tuple(b"".join(b"".join(_rows[(case.name, p % len(case.provers))][k][lo:hi]) for p in range(nb)) for k in range(3))


def scanned(gpu, scan_min):
    gpu.set_option("witness_route", 0)
    gpu.set_option("witness_scan_min", scan_min)


def default_scan_min():
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    return int(re.search(r"#define BPGPU_OPT_WITNESS_SCAN_MIN 21 .*?\(default (\d+);", hdr).group(1))


@pytest.fixture(autouse=True)
def restore(gpu):
    yield
    scanned(gpu, default_scan_min())


@pytest.mark.parametrize("name", NEW + list(GADGETS))
def test_scan_form_equals_the_model_with_and_without_the_scan(gpu, program, name):
    case, w = find(name), program(name)
    n = case.prog.n
    for nb in NBS:
        v, inputs, chi = case.operands(nb)
        want = planes(case, nb)
        for scan_min in (1, 0):
            scanned(gpu, scan_min)
            assert gpu.r1cs_witness_synthesize(w, nb, n, 0, v, inputs, chi) == want, (nb, scan_min)
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


@pytest.mark.parametrize("name", ("mixed", "segments", "chain257", "composite"))
def test_phase_one_then_phase_two_equals_phase_zero(gpu, program, name):
    case, w = find(name), program(name)
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


def test_scanned_shuffle_satisfies_its_circuit_and_a_broken_one_does_not(gpu, program):
    case, w = find("shuffle300"), program("shuffle300")
    prog = case.prog
    assert cc.figures(prog)["longest2"] == 298
    nb = 2
    q, nchi, rp, kd, ix, cf = wc.circuit_csr(case)
    circ = gpu.circuit_create_param(q, nchi, rp, kd, ix, cf, prog.n, prog.m)

    def broken(p):
        v, inputs, chi = case.prover(p + 3)
        v2, inputs2 = case.breaker(v, inputs)
        return v2, inputs2, chi
    try:
        scanned(gpu, 1)
        for which, verdict in ((lambda p: case.prover(p + 3), [1, 1]), (broken, [0, 0])):       # provers 3, 4: random challenges
            v, inputs, chi = case.operands(nb, which)
            got = gpu.r1cs_witness_synthesize(w, nb, prog.n, 0, v, inputs, chi)
            if verdict[0]:
                assert got == tuple(b"".join(wc.mont(x) for p in range(nb) for x in case.want(p + 3)[k]) for k in range(3))
            ok, row, gate, _ = gpu.r1cs_constraints_satisfied(circ, nb, q, *got, v=v, gadget_challenges=chi)
            assert ok == verdict and gate == [-1] * nb                                          # (the gates hold either way)
    finally:
        gpu.circuit_destroy(circ)


def test_option_range_default_and_the_forced_routes(gpu):
    import mpc_bulletproof_amd as mm
    fresh = mm.BpGpu(0)
    try:
        assert fresh.get_option("witness_scan_min") == default_scan_min() >= 16
        assert fresh.get_option("witness_route") == 0
    finally:
        fresh.close()
    for value in (0, 1, 1 << 25):
        gpu.set_option("witness_scan_min", value)
        assert gpu.get_option("witness_scan_min") == value
    for value in (-1, (1 << 25) + 1):
        with pytest.raises(mm.lib.BpGpuError) as e:
            gpu.set_option("witness_scan_min", value)
        assert e.value.code == mm.lib.E_ARG and gpu.get_option("witness_scan_min") == 1 << 25
    with pytest.raises(mm.lib.BpGpuError):
        gpu.set_option("witness_route", 3)
    # a forced route is taken whatever the option says: the same bytes
    case = find("chain257")
    w = gpu.witness_create(*case.prog.create_args())
    try:
        v, inputs, chi = case.operands(3)
        gpu.set_option("witness_scan_min", 1)
        for route in (1, 2):
            gpu.set_option("witness_route", route)
            assert gpu.r1cs_witness_synthesize(w, 3, case.prog.n, 0, v, inputs, chi) == planes(case, 3), route
    finally:
        gpu.witness_destroy(w)


@pytest.mark.parametrize("name", ("shuffle9", "composite"))
def test_one_call_prover_with_the_gadget_scanned(gpu, name):
    """bpgpu_r1cs_prove_fs2 with scan_min = 1: the bytes of _begin / _finish fed the Python-evaluated witness (the comparison of
    tests/test_gpu_prove_fs2_onecall.py, whose model records and helpers this test borrows), accepted by the wire verifier"""
    import oracle_lib as o
    import test_gpu_prove_fs2_onecall as one
    from prove_fs_cases import lg_padded
    gens = gpu.gens_create(o.gens("G", one.CAP), o.gens("H", one.CAP), o.generator(), o.generator(), 8)
    case = wc.case(name)
    n, m, n1 = case.prog.n, case.prog.m, case.prog.phase1
    nb, keys = 2, True
    recs = [one.record(one.ModelGens(one.CAP), name, p) for p in range(nb)]
    cat = lambda key: b"".join(r[key] for r in recs)      # noqa: E731
    plen = 1 + 14 * 32 + (2 * lg_padded(n) + 2) * 32
    circ, w = one.handles(gpu, name, recs[0])
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
