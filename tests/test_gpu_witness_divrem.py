"""BPGPU_GATE_DIVREM on the GPU against Python integers (tests/witness_divrem_cases.py: divmod): every case through the host and
`_dev` forms of bpgpu_r1cs_witness_synthesize with 1, 3 and 65 provers on both forced routes, and with the scan form for the case
with chains; the identity x = q y + r recomputed from the planes that came back; the phases one after the other; the two-phase case
through bpgpu_r1cs_prove_fs2 and the wire verifier; the div-rem gadget through bpgpu_r1cs_prove_values on a context and over a
pool, a prover with a zero divisor rejected; and a non-canonical value."""
import random

import pytest

import oracle_lib as o
import witness_cases as wc
import witness_divrem_cases as dc
from prove_fs_cases import lg_padded

pytestmark = pytest.mark.gpu
pm = wc.pm
N = wc.N
NBS = (1, 3, 65)
ROUTES = (1, 2)          # BPGPU_OPT_WITNESS_ROUTE: a lane per prover, a block per prover
NAMES = [c.name for c in dc.cases()]
CAP = 64
PROOF_ROWS = ("points", "scalars", "wire", "challenges", "states")


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
            made[name] = gpu.witness_create(*dc.case(name).prog.create_args())
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
    """(witness_route, witness_scan_min): the two forced routes, and for the case with chains the library's own choice with every
    chain scanned"""
    return [(route, 0) for route in ROUTES] + ([(0, 1)] if name in dc.CHAINED else [])


class DevBatch:
    """the operands of a batch and three planes in device memory"""

    def __init__(self, gpu, case, nb):
        self.gpu, self.nb, self.n = gpu, nb, case.prog.n
        self.bufs = []
        v, inputs, chi = operands(case, nb)
        self.v, self.inputs, self.chi = (self.up(x) for x in (v, inputs, chi))
        self.planes = [self.up(bytes(32 * nb * self.n)) for _ in range(3)]

    def up(self, data):
        if not data:
            return None
        p = self.gpu.to_device(data)
        self.bufs.append(p)
        return p

    def download(self):
        return tuple(self.gpu.download(p, 32 * self.nb * self.n) for p in self.planes)

    def free(self):
        for p in self.bufs:
            self.gpu.free(p)


def identity_holds(case, nb, got):
    """x = q y + r over the integers and r < y (or y = 0, q = 0), with q and r decoded from the planes that came back and x, y
    from the gates' rows evaluated on those planes: apart from the model's planes"""
    prog = case.prog
    for p in range(min(nb, len(case.provers))):
        v, _, chi = case.prover(p)
        aL, aR, aO = ([wc.md.unmont(plane[32 * (prog.n * p + i):32 * (prog.n * p + i + 1)]) for i in range(prog.n)] for plane in got)
        value = (aL, aR, aO, v)
        for i, (op, _, left, right) in enumerate(prog.gates):
            if op != dc.DIVREM:
                continue
            x, y = (sum(sum((part or 0) * (chi[j - 1] if j else 1) for j, part in enumerate(prog.parts(c))) *
                        (1 if kind == wc.ONE else value[kind][idx]) for kind, idx, c in row) % N for row in (left, right))
            assert x == aL[i] * y + aR[i] and (aR[i] < y or (y == 0 and aL[i] == 0)) and aO[i] == aL[i] * aR[i] % N, (case.name, p, i)


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("name", NAMES)
def test_host_and_dev_forms_equal_divmod(gpu, program, name, nb):
    case, w = dc.case(name), program(name)
    n = case.prog.n
    v, inputs, chi = operands(case, nb)
    want = planes(case, nb)
    dev = DevBatch(gpu, case, nb)
    try:
        for route, scan_min in settings(name):
            gpu.set_option("witness_route", route)
            gpu.set_option("witness_scan_min", scan_min)
            got = gpu.r1cs_witness_synthesize(w, nb, n, 0, v, inputs, chi)
            for k in range(3):
                assert got[k] == want[k], (route, scan_min, "host", "LRO"[k])
            for p in dev.planes:
                gpu.upload(p, bytes(32 * nb * n))
            gpu.r1cs_witness_synthesize_dev(w, nb, 0, *dev.planes, d_v=dev.v, d_inputs=dev.inputs, d_gadget_challenges=dev.chi)
            got = dev.download()
            for k in range(3):
                assert got[k] == want[k], (route, scan_min, "dev", "LRO"[k])
            assert gpu.input_flag() == 0
        identity_holds(case, nb, got)
    finally:
        dev.free()


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("name", NAMES)
def test_phase_one_then_phase_two_equals_phase_zero(gpu, program, name, nb):
    case, w = dc.case(name), program(name)
    n, n1 = case.prog.n, case.prog.phase1
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


@pytest.mark.parametrize("nb", NBS)
def test_two_phase_circuit_is_proved_in_one_call(gpu, gens, program, nb):
    """phase-2 DIVREM gates on the challenge: bpgpu_r1cs_prove_fs2 gives the bytes of bpgpu_r1cs_prove_fs2_begin / _finish fed the
    model's witness on the challenge _begin returned, hands back that witness, and bpgpu_r1cs_verify_batch_wire2 accepts the proofs"""
    name = "dr_two_phase"
    case, w = dc.case(name), program(name)
    prog = case.prog
    n, n1, m = prog.n, prog.phase1, prog.m
    (q, nchi, rp, kd, ix, cf), rows = dc.two_phase_circuit()
    circ = gpu.circuit_create_param(q, 1, rp, kd, ix, cf, n, m)
    rnd = random.Random(616)
    ark = lambda count: b"".join(wc.mont(rnd.randrange(N)) for _ in range(count))      # noqa: E731
    init = b"".join(pm.Transcript(b"div-rem %d" % p).state for p in range(nb))
    v, _, _ = operands(case, nb)
    vb = ark(nb * m)
    bl = [(ark(3), ark(8)) for _ in range(nb)]
    keys = [(bytes(rnd.getrandbits(8) for _ in range(32)), bytes(rnd.getrandbits(8) for _ in range(32))) for _ in range(nb)]
    try:
        _, Vc, states = gpu.r1cs_commit_values(gens, nb, m, v, vb, states=init)
        results = {}
        for route in (0,) + ROUTES:
            gpu.set_option("witness_route", route)
            results[route] = gpu.r1cs_prove_fs2(gens, circ, w, nb, n, m, states=states, gadget_label=dc.LABEL, v=v, v_blinding=vb,
                                                blindings=b"".join(a + b for a, b in bl), vector_keys=b"".join(a + b for a, b in keys),
                                                want_witness=True)
        pts, sc, wire, ch, so, chi, got = results[1]
        assert all(r == results[1] for r in results.values())
        # the model's witness on the challenges the transcript gave
        chis = [int.from_bytes(chi[32 * p:32 * p + 32], "little") for p in range(nb)]
        wits = [prog.evaluate(case.prover(p)[0], (), (chis[p],)) for p in range(nb)]
        part = lambda kk, lo, hi: b"".join(b"".join(wc.mont(x) for x in wits[p][kk][lo:hi]) for p in range(nb))      # noqa: E731
        assert got == tuple(part(kk, 0, n) for kk in range(3))
        for p in range(nb):
            assert dc.rows_hold(rows, wits[p], case.prover(p)[0], (chis[p],)) == -1
            assert any(wits[p][0][i] for i in range(n1, n) if prog.gates[i][0] == dc.DIVREM)       # a quotient that is not zero
        # ... and the two calls around a host that evaluates the gadget
        sess, _, chi2, _ = gpu.r1cs_prove_fs2_begin(gens, circ, nb, n1, states=states, gadget_label=dc.LABEL, blindings=b"".join(a for a, _ in bl),
                                                    a_L=part(0, 0, n1), a_R=part(1, 0, n1), a_O=part(2, 0, n1),
                                                    vector_keys=b"".join(a for a, _ in keys))
        assert chi2 == chi
        assert gpu.r1cs_prove_fs2_finish(gens, circ, sess, nb, n, m, a_L=part(0, n1, n), a_R=part(1, n1, n), a_O=part(2, n1, n),
                                         blindings=b"".join(b for _, b in bl), v_blinding=vb,
                                         vector_keys=b"".join(b for _, b in keys)) == (pts, sc, wire, ch, so)
        plen = 1 + 14 * 32 + (2 * lg_padded(n) + 2) * 32
        assert len(wire) == nb * plen
        assert gpu.r1cs_verify_batch_wire2(gens, circ, nb, n1, plen, dc.LABEL, wire, Vc, init) == [1] * nb
    finally:
        gpu.circuit_destroy(circ)


def gadget_operands(case, nb, seed):
    prog = case.prog
    rnd = random.Random(seed)
    ark = lambda count: b"".join(wc.mont(rnd.randrange(N)) for _ in range(count))      # noqa: E731
    v, _, _ = operands(case, nb)
    return dict(init_states=b"".join(pm.Transcript(b"div-rem gadget %d" % p).state for p in range(nb)), v=v, v_blinding=ark(nb * prog.m),
                inputs=None, blindings=ark(8 * nb), gadget_label=None, vector_keys=bytes(rnd.getrandbits(8) for _ in range(32 * nb)))


def check_gadget_result(gpu, gens, circ, case, nb, got, ops):
    """ok, first_bad_row and first_bad_gate as the model says, the planes divmod's, the rejected provers' proof rows zero bytes, and
    the wire verifier accepts exactly the accepted provers"""
    prog = case.prog
    verdicts = [dc.gadget_verdict(case, p % len(case.provers)) for p in range(nb)]
    assert (got.ok, got.first_bad_row, got.first_bad_gate) == tuple([vd[k] for vd in verdicts] for k in range(3))
    assert got.planes == planes(case, nb)
    k = lg_padded(prog.n)
    per = dict(points=64 * (11 + 2 * k), scalars=160, wire=1 + 11 * 32 + (2 * k + 2) * 32, challenges=32 * (5 + k), states=32)
    for p in range(nb):
        for field in PROOF_ROWS:
            row = getattr(got, field)[per[field] * p:per[field] * (p + 1)]
            assert (row == bytes(per[field])) == (not got.ok[p]), (p, field)
    assert gpu.r1cs_verify_batch_wire(gens, circ, nb, prog.n, per["wire"], got.wire, got.V_compressed, ops["init_states"]) == got.ok


@pytest.mark.parametrize("nb", NBS)
def test_gadget_through_prove_values(gpu, gens, program, nb):
    """the div-rem gadget from the committed a, b in one call: b = 1, b > a, b | a and b = 2^16 - 1 are proved, b = 0 is rejected by
    the range check (nb = 1 holds an accepted prover only; 3 accepted ones; 65 both kinds)"""
    name = "dr_gadget"
    case, w = dc.case(name), program(name)
    prog = case.prog
    q, nchi, rp, kd, ix, cf = wc.circuit_csr(case)
    assert nchi == 0
    circ = gpu.circuit_create(rp, kd, ix, cf, prog.n, prog.m)
    ops = gadget_operands(case, nb, 717)
    try:
        results = {}
        for route in (0,) + ROUTES:
            gpu.set_option("witness_route", route)
            results[route] = gpu.r1cs_prove_values(gens, circ, w, nb, prog.n, prog.m, want_witness=True, **ops)
        got = results[1]
        assert all(tuple(r) == tuple(got) for r in results.values())
        check_gadget_result(gpu, gens, circ, case, nb, got, ops)
        assert (0 in got.ok) == (nb > 4) and 1 in got.ok
    finally:
        gpu.circuit_destroy(circ)


def test_gadget_through_the_pool(gpu, gens):
    """bpgpu_pool_witness_create with bpgpu_pool_r1cs_prove_values on a {0, 0} pool: the five provers, the last one rejected"""
    import mpc_bulletproof_amd as m
    name = "dr_gadget"
    case = dc.case(name)
    prog = case.prog
    nb = len(case.provers)
    q, nchi, rp, kd, ix, cf = wc.circuit_csr(case)
    ops = gadget_operands(case, nb, 818)
    pool = m.BpPool([0, 0])
    try:
        pgens = pool.gens_create(o.gens("G", CAP), o.gens("H", CAP), o.generator(), o.generator(), 8)
        circ = pool.circuit_create(rp, kd, ix, cf, prog.n, prog.m)
        w = pool.witness_create(*prog.create_args())
        got = pool.r1cs_prove_values(pgens, circ, w, nb, prog.n, prog.m, want_witness=True, **ops)
        single = gpu.circuit_create(rp, kd, ix, cf, prog.n, prog.m)
        try:
            check_gadget_result(gpu, gens, single, case, nb, got, ops)
        finally:
            gpu.circuit_destroy(single)
        assert got.ok == [1, 1, 1, 1, 0]
        pool.witness_destroy(w)
        pool.circuit_destroy(circ)
        pool.gens_destroy(pgens)
    finally:
        pool.close()


def test_non_canonical_value_is_flagged(gpu, program):
    """a value that is the group order: BPGPU_E_ARG in the host form, the input flag in the `_dev` form, and the context synthesizes
    as before afterwards"""
    import mpc_bulletproof_amd as mm
    case, w = dc.case("dr_gadget"), program("dr_gadget")
    n, m, nb = case.prog.n, case.prog.m, 3
    v, inputs, chi = operands(case, nb)
    want = planes(case, nb)
    bad_v = v[:32 * (m + 1)] + N.to_bytes(32, "little") + v[32 * (m + 2):]           # the divisor of prover 1 := the group order
    with pytest.raises(mm.lib.BpGpuError) as e:
        gpu.r1cs_witness_synthesize(w, nb, n, 0, bad_v, inputs, chi)
    assert e.value.code == mm.lib.E_ARG
    dev = DevBatch(gpu, case, nb)
    try:
        gpu.upload(dev.v, bad_v)
        gpu.r1cs_witness_synthesize_dev(w, nb, 0, *dev.planes, d_v=dev.v)
        assert gpu.input_flag() == 1
        gpu.upload(dev.v, v)
        gpu.r1cs_witness_synthesize_dev(w, nb, 0, *dev.planes, d_v=dev.v)
        assert gpu.input_flag() == 0 and dev.download() == want
    finally:
        dev.free()
    assert gpu.r1cs_witness_synthesize(w, nb, n, 0, v, inputs, chi) == want


def test_mpc_witness_begin_refuses_the_phases_with_a_divrem_gate(gpu, program):
    import mpc_bulletproof_amd as mm
    case, w = dc.case("dr_two_phase"), program("dr_two_phase")
    prog = case.prog
    nb = 1
    v = bytes(32 * nb * 3 * prog.m)
    chi = bytes(32 * nb)
    held = bytes(32 * nb * 3 * prog.n)
    for phase, kw in ((0, dict(gadget_challenges=chi)), (2, dict(gadget_challenges=chi, a_L=held, a_R=held, a_O=held))):
        with pytest.raises(mm.lib.BpGpuError) as e:
            gpu.mpc_witness_begin(w, nb, phase, v=v, **kw)
        assert e.value.code == mm.lib.E_ARG, phase
    # phase 1 of this program holds no DIVREM gate: it is evaluated as before
    s = gpu.mpc_witness_begin(w, nb, 1, v=v)
    assert s is not None and gpu.mpc_witness_levels_left(s) == 1
    gpu.mpc_witness_destroy(s)
