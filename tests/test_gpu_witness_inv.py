"""BPGPU_GATE_INV on the GPU against the helper's witnesses (tests/witness_inv_cases.py): every case through the host and `_dev`
forms with 1, 3 and 65 provers on both forced routes, and with the scan form enabled for the cases that have a chain; the phases one
after the other; the chain commit -> synthesize -> check -> prove on one set of device buffers; and a two-phase circuit proved by
bpgpu_r1cs_prove_fs2 in one call."""
import ctypes as C
import random

import pytest

import oracle_lib as o
import witness_cases as wc
import witness_inv_cases as ic

pytestmark = pytest.mark.gpu
pm = wc.pm
N = wc.N
NBS = (1, 3, 65)
ROUTES = (1, 2)          # BPGPU_OPT_WITNESS_ROUTE: a lane per prover (one inversion per gate), a block per prover (one per thread and level)
NAMES = [c.name for c in ic.cases()]
CAP = 32


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
            made[name] = gpu.witness_create(*ic.case(name).prog.create_args())
        return made[name]
    yield get
    for w in made.values():
        gpu.witness_destroy(w)


@pytest.fixture(scope="module")
def gens(gpu):
    g = gpu.gens_create(o.gens("G", CAP), o.gens("H", CAP), o.generator(), o.generator(), 8)
    yield g
    gpu.gens_destroy(g)


@pytest.fixture(autouse=True)
def restore(gpu):
    scan_min = gpu.get_option("witness_scan_min")
    yield
    gpu.set_option("witness_route", 0)
    gpu.set_option("witness_scan_min", scan_min)


_rows, _ops = {}, {}


def planes(case, nb, lo=0, hi=None):
    """the expected planes of a batch, ark form (a prover's rows encoded once, however often the batch repeats it)"""
    hi = case.prog.n if hi is None else hi
    for p in range(min(nb, len(case.provers))):
        if (case.name, p) not in _rows:
            _rows[(case.name, p)] = tuple([wc.mont(x) for x in plane] for plane in case.want(p))
    return tuple(b"".join(b"".join(_rows[(case.name, p % len(case.provers))][k][lo:hi]) for p in range(nb)) for k in range(3))


def operands(case, nb):
    if (case.name, nb) not in _ops:
        _ops[(case.name, nb)] = case.operands(nb)
    return _ops[(case.name, nb)]


def settings(name):
    """(witness_route, witness_scan_min): the two forced routes, and for a case with a chain the library's own choice with every
    chain scanned"""
    return [(route, 0) for route in ROUTES] + ([(0, 1)] if name in ic.CHAINED else [])


class DevBatch:
    """the operands of a batch and three planes in device memory"""

    def __init__(self, gpu, case, nb, ops=None):
        self.gpu, self.nb, self.n = gpu, nb, case.prog.n
        self.bufs = []
        v, inputs, chi = ops if ops is not None else operands(case, nb)
        self.v, self.inputs, self.chi = (self.up(x) for x in (v, inputs, chi))
        self.planes = [self.up(bytes(32 * nb * self.n)) for _ in range(3)]

    def up(self, data):
        if not data:
            return None
        p = self.gpu.to_device(data)
        self.bufs.append(p)
        return p

    def malloc(self, nbytes):
        p = self.gpu.malloc(nbytes)
        self.bufs.append(p)
        return p

    def download(self):
        return tuple(self.gpu.download(p, 32 * self.nb * self.n) for p in self.planes)

    def free(self):
        for p in self.bufs:
            self.gpu.free(p)


@pytest.mark.parametrize("name", NAMES)
def test_host_and_dev_forms_equal_the_helper(gpu, program, name):
    case, w = ic.case(name), program(name)
    n = case.prog.n
    for nb in NBS:
        v, inputs, chi = operands(case, nb)
        want = planes(case, nb)
        dev = DevBatch(gpu, case, nb)
        try:
            for route, scan_min in settings(name):
                gpu.set_option("witness_route", route)
                gpu.set_option("witness_scan_min", scan_min)
                assert gpu.r1cs_witness_synthesize(w, nb, n, 0, v, inputs, chi) == want, (nb, route, scan_min, "host")
                for p in dev.planes:
                    gpu.upload(p, bytes(32 * nb * n))
                gpu.r1cs_witness_synthesize_dev(w, nb, 0, *dev.planes, d_v=dev.v, d_inputs=dev.inputs, d_gadget_challenges=dev.chi)
                assert dev.download() == want, (nb, route, scan_min, "dev")
                assert gpu.input_flag() == 0
        finally:
            dev.free()


@pytest.mark.parametrize("name", NAMES)
def test_phase_one_then_phase_two_equals_phase_zero(gpu, program, name):
    case, w = ic.case(name), program(name)
    n, n1, nb = case.prog.n, case.prog.phase1, 3
    v, inputs, chi = operands(case, nb)
    want = planes(case, nb)
    marker = wc.mont(12345)
    for route, scan_min in settings(name):
        gpu.set_option("witness_route", route)
        gpu.set_option("witness_scan_min", scan_min)
        held = tuple(marker * (nb * n) for _ in range(3))
        first = gpu.r1cs_witness_synthesize(w, nb, n, 1, v, inputs, None, *held)
        for plane, full in zip(first, want):
            for p in range(nb):
                row = plane[32 * n * p:32 * n * (p + 1)]
                assert row[:32 * n1] == full[32 * n * p:32 * (n * p + n1)] and row[32 * n1:] == marker * (n - n1), (route, p)
        assert gpu.r1cs_witness_synthesize(w, nb, n, 2, v, inputs, chi, *first) == want, (route, scan_min)
        dev = DevBatch(gpu, case, nb)
        try:
            gpu.r1cs_witness_synthesize_dev(w, nb, 1, *dev.planes, d_v=dev.v, d_inputs=dev.inputs)
            gpu.r1cs_witness_synthesize_dev(w, nb, 2, *dev.planes, d_v=dev.v, d_inputs=dev.inputs, d_gadget_challenges=dev.chi)
            assert dev.download() == want, (route, scan_min)
        finally:
            dev.free()


def with_commitments(points, V, nb, m, k):
    """the verifier's operand layout: V_0..V_{m-1} (nb x m x 64 B) inserted after the six A / S points of each proof"""
    nvar, out = 11 + 2 * k, b""
    for p in range(nb):
        pp = points[64 * nvar * p:64 * nvar * (p + 1)]
        out += pp[:6 * 64] + V[64 * m * p:64 * m * (p + 1)] + pp[6 * 64:]
    return out


def test_commit_synthesize_check_prove_chain_on_device_buffers(gpu, gens, program):
    """bpgpu_r1cs_commit_values_dev -> bpgpu_r1cs_witness_synthesize_dev -> bpgpu_r1cs_constraints_satisfied_dev ->
    bpgpu_r1cs_prove_fs_dev on one set of buffers, nothing waited for in between: every prover is accepted and its proof verifies;
    with one prover's committed `is not zero` claim false, exactly that one is reported, with its first failing row"""
    name = "inv_is_zero"
    case, w = ic.case(name), program(name)
    prog = case.prog
    n, m, nb, bad = prog.n, prog.m, 5, 3
    k = max(n - 1, 0).bit_length()
    nvar = 11 + 2 * k
    q, nchi, rp, kd, ix, cf = wc.circuit_csr(case)
    assert nchi == 0
    circ = gpu.circuit_create(rp, kd, ix, cf, n, m)
    rnd = random.Random(515)
    init = b"".join(pm.Transcript(b"is-zero %d" % p).state for p in range(nb))

    def broken(p):
        v, inputs, chi = case.prover(p)
        if p != bad:
            return v, inputs, chi
        v2, inputs2 = case.breaker(v, inputs)
        return v2, inputs2, chi
    # the first row that fails for the false claim, from the model: the constraint b_0 - claim_0
    pv = wc.Case(name, prog, [broken(bad)], case.gadget).model(0)
    first_bad = next(r for r, lc in enumerate(pv.constraints) if pv.eval(lc))
    try:
        for which, verdict in ((None, [1] * nb), (broken, [0 if p == bad else 1 for p in range(nb)])):
            dev = DevBatch(gpu, case, nb, case.operands(nb, which))
            try:
                d_vb = dev.up(b"".join(wc.mont(rnd.randrange(N)) for _ in range(nb * m)))
                d_bl = dev.up(b"".join(wc.mont(rnd.randrange(N)) for _ in range(8 * nb)))
                d_keys = dev.up(bytes(rnd.getrandbits(8) for _ in range(32 * nb)))
                d_init = dev.up(init)
                d_V, d_st, d_ok, d_row = dev.malloc(64 * nb * m), dev.malloc(32 * nb), dev.malloc(4 * nb), dev.malloc(8 * nb)
                d_pts, d_sc = dev.malloc(64 * nb * nvar), dev.malloc(160 * nb)
                gpu.r1cs_commit_values_dev(gens, nb, m, dev.v, d_vb, d_init, d_V, None, d_st)
                gpu.r1cs_witness_synthesize_dev(w, nb, 0, *dev.planes, d_v=dev.v)
                gpu.r1cs_constraints_satisfied_dev(circ, nb, *dev.planes, d_ok, d_v=dev.v, d_first_bad_row=d_row)
                gpu.r1cs_prove_fs_dev(gens, circ, nb, d_st, *dev.planes, d_bl, d_pts, d_sc, d_v_blinding=d_vb, d_vector_keys=d_keys)
                assert gpu.input_flag() == 0
                ok = list((C.c_int32 * nb).from_buffer_copy(gpu.download(d_ok, 4 * nb)))
                rows = list((C.c_int64 * nb).from_buffer_copy(gpu.download(d_row, 8 * nb)))
                assert ok == verdict and rows == [-1 if x else first_bad for x in verdict]
                assert dev.download() == planes(case, nb)           # the witness does not depend on the claims
                full = with_commitments(gpu.download(d_pts, 64 * nb * nvar), gpu.download(d_V, 64 * nb * m), nb, m, k)
                assert gpu.r1cs_verify_batch_fs(gens, circ, nb, n, k, m, init, full, gpu.download(d_sc, 160 * nb))[0] == verdict
            finally:
                dev.free()
    finally:
        gpu.circuit_destroy(circ)


def test_two_phase_circuit_is_proved_in_one_call(gpu, gens, program):
    """the is-zero gadget in phase 1, a shuffle and an INV gate on the challenge in phase 2: bpgpu_r1cs_prove_fs2 gives the bytes of
    bpgpu_r1cs_prove_fs2_begin / _finish fed the helper's witness on the challenge _begin returned, hands back that witness, and
    bpgpu_r1cs_verify_batch_fs2 accepts the proofs"""
    name = "inv_two_phase"
    case, w = ic.case(name), program(name)
    prog = case.prog
    n, n1, m, nb = prog.n, prog.phase1, prog.m, 5
    n2 = n - n1
    k = max(n - 1, 0).bit_length()
    q, nchi, rp, kd, ix, cf = wc.circuit_csr(case)
    assert nchi == 1
    circ = gpu.circuit_create_param(q, 1, rp, kd, ix, cf, n, m)
    rnd = random.Random(616)
    ark = lambda count: b"".join(wc.mont(rnd.randrange(N)) for _ in range(count))      # noqa: E731
    init = b"".join(pm.Transcript(b"two-phase %d" % p).state for p in range(nb))
    v, inputs, _ = operands(case, nb)
    vb = ark(nb * m)
    bl = [(ark(3), ark(8)) for _ in range(nb)]
    keys = [(bytes(rnd.getrandbits(8) for _ in range(32)), bytes(rnd.getrandbits(8) for _ in range(32))) for _ in range(nb)]
    try:
        V, _, states = gpu.r1cs_commit_values(gens, nb, m, v, vb, init, want_compressed=False)
        results = {}
        for route, scan_min in settings(name) + [(0, gpu.get_option("witness_scan_min"))]:
            gpu.set_option("witness_route", route)
            gpu.set_option("witness_scan_min", scan_min)
            results[(route, scan_min)] = gpu.r1cs_prove_fs2(gens, circ, w, nb, n, m, states=states, gadget_label=ic.LABEL, v=v, v_blinding=vb,
                                                            blindings=b"".join(a + b for a, b in bl),
                                                            vector_keys=b"".join(a + b for a, b in keys), want_witness=True)
        pts, sc, wire, ch, so, chi, got = results[(1, 0)]
        assert all(r == results[(1, 0)] for r in results.values())
        # the helper's witness on the challenges the transcript gave
        chis = [int.from_bytes(chi[32 * p:32 * p + 32], "little") for p in range(nb)]
        wits = [prog.evaluate(case.prover(p)[0], (), (chis[p],)) for p in range(nb)]
        part = lambda kk, lo, hi: b"".join(b"".join(wc.mont(x) for x in wits[p][kk][lo:hi]) for p in range(nb))      # noqa: E731
        assert got == tuple(part(kk, 0, n) for kk in range(3))
        assert any(wits[p][0][n - 1] != 0 for p in range(nb))              # the INV gate on the challenge: v_0 - z
        # ... and the two calls around a host that evaluates the gadget
        sess, _, chi2, _ = gpu.r1cs_prove_fs2_begin(gens, circ, nb, n1, states=states, gadget_label=ic.LABEL, blindings=b"".join(a for a, _ in bl),
                                                    a_L=part(0, 0, n1), a_R=part(1, 0, n1), a_O=part(2, 0, n1),
                                                    vector_keys=b"".join(a for a, _ in keys))
        assert chi2 == chi
        assert gpu.r1cs_prove_fs2_finish(gens, circ, sess, nb, n, m, a_L=part(0, n1, n), a_R=part(1, n1, n), a_O=part(2, n1, n),
                                         blindings=b"".join(b for _, b in bl), v_blinding=vb,
                                         vector_keys=b"".join(b for _, b in keys)) == (pts, sc, wire, ch, so)
        assert n2 == 2 * (ic.TWO_PHASE_K - 1) + 1
        full = with_commitments(pts, V, nb, m, k)
        ok = gpu.r1cs_verify_batch_fs2(gens, circ, nb, n1, k, m, 1, init, ic.LABEL, full, sc)
        assert ok[0] == [1] * nb and ok[3] == chi
        okc, row, gate, _ = gpu.r1cs_constraints_satisfied(circ, nb, q, *got, v=v, gadget_challenges=chi)
        assert okc == [1] * nb and row == [-1] * nb and gate == [-1] * nb
    finally:
        gpu.circuit_destroy(circ)


def test_mpc_witness_begin_refuses_the_phases_with_an_inv_gate(gpu, program):
    import mpc_bulletproof_amd as mm
    case, w = ic.case("inv_chi"), program("inv_chi")
    prog = case.prog
    nb = 1
    v = bytes(32 * nb * 3 * prog.m)
    chi = bytes(32 * nb)
    held = bytes(32 * nb * 3 * prog.n)
    for phase, kw in ((0, dict(gadget_challenges=chi)), (1, {}), (2, dict(gadget_challenges=chi, a_L=held, a_R=held, a_O=held))):
        with pytest.raises(mm.lib.BpGpuError) as e:
            gpu.mpc_witness_begin(w, nb, phase, v=v, **kw)
        assert e.value.code == mm.lib.E_ARG, phase
    # phase 1 of a program whose INV gates are all in phase 2 is evaluated as before
    two = ic.Program(1, nchi=1)
    two.mul([(wc.V, 0, 1)], [(wc.V, 0, 1)])
    two.end_phase1()
    two.inv([(wc.O, 0, (None, 1))])
    h = gpu.witness_create(*two.create_args())
    try:
        s = gpu.mpc_witness_begin(h, nb, 1, v=bytes(32 * 3))
        assert s is not None and gpu.mpc_witness_levels_left(s) == 1
        gpu.mpc_witness_destroy(s)
        with pytest.raises(mm.lib.BpGpuError):
            gpu.mpc_witness_begin(h, nb, 2, v=bytes(32 * 3), gadget_challenges=chi, a_L=bytes(192), a_R=bytes(192), a_O=bytes(192))
    finally:
        gpu.witness_destroy(h)
