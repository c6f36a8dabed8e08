"""bpgpu_r1cs_witness_synthesize / _dev on the GPU against the helper's witnesses (tests/witness_cases.py): every case, 1, 3 and 65
provers, both launch forms; the phases one after the other; the chain commit -> synthesize -> check on one set of device buffers; and
a non-canonical operand."""
import ctypes as C

import pytest

import oracle_lib as o
import witness_cases as wc

pytestmark = pytest.mark.gpu
N = wc.N
NBS = (1, 3, 65)
ROUTES = (1, 2)          # BPGPU_OPT_WITNESS_ROUTE: a lane per prover, a block per prover
NAMES = [c.name for c in wc.cases()]
GADGETS = [c.name for c in wc.gadget_cases()]


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
            made[name] = gpu.witness_create(*wc.case(name).prog.create_args())
        return made[name]
    yield get
    for w in made.values():
        gpu.witness_destroy(w)


class DevBatch:
    """the operands of a batch and three planes in device memory"""

    def __init__(self, gpu, case, nb, which=None):
        self.gpu, self.nb, self.n = gpu, nb, case.prog.n
        self.bufs = []
        v, inputs, chi = case.operands(nb, which)
        self.v, self.inputs, self.chi = (self._up(x) for x in (v, inputs, chi))
        self.planes = [self._up(bytes(32 * nb * self.n)) for _ in range(3)]

    def _up(self, data):
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
def test_host_and_dev_forms_equal_the_helper_on_both_routes(gpu, program, name):
    case, w = wc.case(name), program(name)
    n = case.prog.n
    try:
        for nb in NBS:
            v, inputs, chi = case.operands(nb)
            want = case.planes(nb)
            dev = DevBatch(gpu, case, nb)
            try:
                for route in ROUTES:
                    gpu.set_option("witness_route", route)
                    assert gpu.r1cs_witness_synthesize(w, nb, n, 0, v, inputs, chi) == want, (nb, route, "host")
                    for p in dev.planes:
                        gpu.upload(p, bytes(32 * nb * n))
                    gpu.r1cs_witness_synthesize_dev(w, nb, 0, *dev.planes, d_v=dev.v, d_inputs=dev.inputs, d_gadget_challenges=dev.chi)
                    assert dev.download() == want, (nb, route, "dev")
                    assert gpu.input_flag() == 0
            finally:
                dev.free()
    finally:
        gpu.set_option("witness_route", 0)
    # the route the plan takes gives the same bytes
    v, inputs, chi = case.operands(3)
    assert gpu.r1cs_witness_synthesize(w, 3, n, 0, v, inputs, chi) == case.planes(3)


@pytest.mark.parametrize("name", NAMES)
def test_phase_one_then_phase_two_equals_phase_zero(gpu, program, name):
    case, w = wc.case(name), program(name)
    n, n1, nb = case.prog.n, case.prog.phase1, 3
    v, inputs, chi = case.operands(nb)
    want = case.planes(nb)
    marker = wc.mont(12345)
    try:
        for route in ROUTES:
            gpu.set_option("witness_route", route)
            # phase 1 leaves the second phase's multipliers as the caller holds them
            held = tuple(marker * (nb * n) for _ in range(3))
            first = gpu.r1cs_witness_synthesize(w, nb, n, 1, v, inputs, None, *held)
            for plane, full in zip(first, want):
                for p in range(nb):
                    row = plane[32 * n * p:32 * n * (p + 1)]
                    assert row[:32 * n1] == full[32 * n * p:32 * (n * p + n1)] and row[32 * n1:] == marker * (n - n1), (route, p)
            assert gpu.r1cs_witness_synthesize(w, nb, n, 2, v, inputs, chi, *first) == want, route
            # the same on device buffers, the two calls enqueued back to back
            dev = DevBatch(gpu, case, nb)
            try:
                gpu.r1cs_witness_synthesize_dev(w, nb, 1, *dev.planes, d_v=dev.v, d_inputs=dev.inputs)
                gpu.r1cs_witness_synthesize_dev(w, nb, 2, *dev.planes, d_v=dev.v, d_inputs=dev.inputs, d_gadget_challenges=dev.chi)
                assert dev.download() == want, route
            finally:
                dev.free()
    finally:
        gpu.set_option("witness_route", 0)


@pytest.fixture(scope="module")
def gens(gpu):
    g = gpu.gens_create(o.gens("G", 16), o.gens("H", 16), o.generator(), o.generator(), 8)
    yield g
    gpu.gens_destroy(g)


@pytest.mark.parametrize("name", GADGETS)
def test_commit_synthesize_check_chain_on_device_buffers(gpu, gens, program, name):
    """bpgpu_r1cs_commit_values_dev -> bpgpu_r1cs_witness_synthesize_dev -> bpgpu_r1cs_constraints_satisfied_dev on one set of buffers,
    nothing waited for in between: every prover is accepted; with one prover's input changed, exactly that one is rejected"""
    case, w = wc.case(name), program(name)
    prog = case.prog
    nb, bad = 5, 3
    q, nchi, rp, kd, ix, cf = wc.circuit_csr(case)
    circ = gpu.circuit_create_param(q, nchi, rp, kd, ix, cf, prog.n, prog.m) if nchi else gpu.circuit_create(rp, kd, ix, cf, prog.n, prog.m)

    def broken(p):
        v, inputs, chi = case.prover(p)
        if p != bad:
            return v, inputs, chi
        v2, inputs2 = case.breaker(v, inputs)
        return v2, inputs2, chi
    try:
        for which, verdict in ((None, [1] * nb), (broken, [0 if p == bad else 1 for p in range(nb)])):
            dev = DevBatch(gpu, case, nb, which)
            try:
                d_vb = dev._up(b"".join(wc.mont(7 + i) for i in range(nb * prog.m)))
                d_Vc, d_ok = dev.malloc(32 * nb * prog.m), dev.malloc(4 * nb)
                gpu.r1cs_commit_values_dev(gens, nb, prog.m, dev.v, d_vb, d_V_compressed=d_Vc)
                gpu.r1cs_witness_synthesize_dev(w, nb, 0, *dev.planes, d_v=dev.v, d_inputs=dev.inputs, d_gadget_challenges=dev.chi)
                gpu.r1cs_constraints_satisfied_dev(circ, nb, *dev.planes, d_ok, d_v=dev.v, d_gadget_challenges=dev.chi)
                ok = list((C.c_int32 * nb).from_buffer_copy(gpu.download(d_ok, 4 * nb)))
                assert ok == verdict, name
                assert gpu.input_flag() == 0
            finally:
                dev.free()
    finally:
        gpu.circuit_destroy(circ)


def test_non_canonical_limb_is_refused_or_flagged(gpu, program):
    import mpc_bulletproof_amd as mm
    case, w = wc.case("composite"), program("composite")
    n, nb = case.prog.n, 3
    v, inputs, chi = case.operands(nb)
    want = case.planes(nb)
    m = case.prog.m
    bad_v = v[:32 * (m + 2)] + N.to_bytes(32, "little") + v[32 * (m + 3):]           # a value of prover 1 := the group order
    bad_in = inputs[:64] + (b"\xff" * 32) + inputs[96:]
    bad_chi = chi[:32] + N.to_bytes(32, "little") + chi[64:]
    for over in (dict(v=bad_v), dict(inputs=bad_in), dict(gadget_challenges=bad_chi)):
        ops = dict(dict(v=v, inputs=inputs, gadget_challenges=chi), **over)
        with pytest.raises(mm.lib.BpGpuError) as e:
            gpu.r1cs_witness_synthesize(w, nb, n, 0, **ops)
        assert e.value.code == mm.lib.E_ARG, list(over)
    dev = DevBatch(gpu, case, nb)
    try:
        gpu.upload(dev.v, bad_v)
        gpu.r1cs_witness_synthesize_dev(w, nb, 0, *dev.planes, d_v=dev.v, d_inputs=dev.inputs, d_gadget_challenges=dev.chi)
        assert gpu.input_flag() == 1
        gpu.upload(dev.v, v)
        gpu.r1cs_witness_synthesize_dev(w, nb, 0, *dev.planes, d_v=dev.v, d_inputs=dev.inputs, d_gadget_challenges=dev.chi)
        assert gpu.input_flag() == 0 and dev.download() == want
    finally:
        dev.free()
    # the refused calls left nothing behind: the context synthesizes as before
    assert gpu.r1cs_witness_synthesize(w, nb, n, 0, v, inputs, chi) == want
    # phase 2 on planes whose first phase is not canonical
    first = gpu.r1cs_witness_synthesize(w, nb, n, 1, v, inputs, None)
    spoiled = (N.to_bytes(32, "little") + first[0][32:],) + first[1:]
    with pytest.raises(mm.lib.BpGpuError) as e:
        gpu.r1cs_witness_synthesize(w, nb, n, 2, v, inputs, chi, *spoiled)
    assert e.value.code == mm.lib.E_ARG


def test_refusals_on_a_live_context(gpu, program):
    import mpc_bulletproof_amd as mm
    E = mm.lib
    case, w = wc.case("composite"), program("composite")
    n, nb = case.prog.n, 2
    v, inputs, chi = case.operands(nb)

    def code(**kw):
        try:
            gpu.r1cs_witness_synthesize(w, nb, n, **dict(dict(phase=0, v=v, inputs=inputs, gadget_challenges=chi), **kw))
        except E.BpGpuError as e:
            return e.code
        return 0
    assert code() == 0
    assert code(phase=3) == E.E_ARG and code(phase=-1) == E.E_ARG
    assert code(v=None) == E.E_ARG and code(inputs=None) == E.E_ARG and code(gadget_challenges=None) == E.E_ARG
    assert code(phase=1) == E.E_ARG                                   # challenges where phase 1 runs alone
    assert code(phase=1, gadget_challenges=None) == 0
    with pytest.raises(E.BpGpuError):
        gpu.set_option("witness_route", 3)
    numeric = program("example")
    ex = wc.case("example")
    with pytest.raises(E.BpGpuError) as e:
        gpu.r1cs_witness_synthesize(numeric, 1, 1, 0, ex.operands(1)[0], None, chi[:32])
    assert e.value.code == E.E_ARG                                    # challenges given to a numeric program
    assert gpu.r1cs_witness_synthesize(w, 0, n, 0, None, None, chi) == (b"", b"", b"")      # nb == 0
    assert code() == 0
