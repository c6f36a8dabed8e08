"""bpgpu_r1cs_prove_values / _dev: commitments, verdicts and proofs from the provers' committed values in ONE call, against the chain
of existing host-form calls it replaces (tests/prove_values_cases.py: chain) -- byte for byte on every output, under every witness
route, in the `_dev` form, with a rejected prover among five (its proof rows are zero bytes, the others' untouched), with a
non-canonical limb, and the wire proofs verified from exactly what the call returned.  The `_dev` form runs the same grid, and the
rejected prover as well: its rows of the caller's device buffers are cleared without the host reading ok."""
import pytest

import oracle_lib as o
import prove_values_cases as pc

pytestmark = pytest.mark.gpu
N = pc.N
CAP = pc.CAP
NAMES = pc.ONE_PHASE + pc.TWO_PHASE
PROOF_ROWS = ("points", "scalars", "wire", "challenges", "states")


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gens(gpu):
    g = gpu.gens_create(o.gens("G", CAP), o.gens("H", CAP), o.generator(), o.generator(), 8)     # capacity 16, window 8
    yield g
    gpu.gens_destroy(g)


@pytest.fixture(scope="module")
def made(gpu):
    """(circuit, program) per case, created once"""
    h = {}

    def get(name):
        if name not in h:
            h[name] = pc.handles(gpu, name)
        return h[name]
    yield get
    for circ, w in h.values():
        gpu.witness_destroy(w)
        gpu.circuit_destroy(circ)


def one_call(gpu, gens, circ, w, name, nb, ops, **kw):
    prog = pc.case(name).prog
    return gpu.r1cs_prove_values(gens, circ, w, nb, prog.n, prog.m, want_witness=True, **dict(ops, **kw))


def verify(gpu, gens, circ, name, nb, got, ops):
    """the wire verifier on exactly what the call returned: V_compressed, plus the init_states that went in"""
    prog = pc.case(name).prog
    if pc.two_phase(name):
        return gpu.r1cs_verify_batch_wire2(gens, circ, nb, prog.phase1, pc.proof_len(name), pc.LABEL, got.wire, got.V_compressed, ops["init_states"])
    return gpu.r1cs_verify_batch_wire(gens, circ, nb, prog.n, pc.proof_len(name), got.wire, got.V_compressed, ops["init_states"])


@pytest.mark.parametrize("nb", (1, 5))
@pytest.mark.parametrize("keys", (False, True), ids=("explicit", "keys"))
@pytest.mark.parametrize("name", NAMES)
def test_host_form_equals_the_chain_under_every_route_and_verifies(gpu, gens, made, name, keys, nb):
    circ, w = made(name)
    ops = pc.operands(name, nb, keys)
    want = pc.chain(gpu, gens, circ, w, name, nb, ops)
    assert want[0] == [1] * nb and want[1] == [-1] * nb and want[2] == [-1] * nb
    try:
        for route in (0, 1, 2):
            gpu.set_option("witness_route", route)
            got = one_call(gpu, gens, circ, w, name, nb, ops)
            for field, a, b in zip(pc.FIELDS, got, want):
                assert a == b, (route, field)
    finally:
        gpu.set_option("witness_route", 0)
    assert len(got.wire) == nb * pc.proof_len(name) and got.wire[0] == (1 if pc.two_phase(name) else 0)
    assert verify(gpu, gens, circ, name, nb, got, ops) == [1] * nb
    # the optional results left out: the required ones are the same bytes
    prog = pc.case(name).prog
    less = gpu.r1cs_prove_values(gens, circ, w, nb, prog.n, prog.m, want_wire=False, **ops)
    assert less.wire is None and less.planes is None and (less.ok, less.points, less.scalars) == (got.ok, got.points, got.scalars)


class Dev:
    """the operands of a batch and every result on bpgpu_malloc buffers"""

    def __init__(self, gpu, name, nb, ops):
        self.gpu, self.name, self.nb, self.ops = gpu, name, nb, ops
        self.per = pc.row_bytes(name)
        self.names = [f for f in pc.FIELDS if f != "planes" and (f != "chi" or pc.two_phase(name))]
        self.d = {key: gpu.to_device(val) for key, val in ops.items() if val is not None and key != "gadget_label"}
        self.out = {key: gpu.malloc(nb * self.per[key]) for key in self.names + ["a_L", "a_R", "a_O"]}

    def run(self, gens, circ, w, d_out=None):
        prog = pc.case(self.name).prog
        keys = ("init_states", "v", "v_blinding", "inputs", "blindings", "vector_keys", "s_L", "s_R")
        self.gpu.r1cs_prove_values(gens, circ, w, self.nb, prog.n, prog.m, dev=True, d_out=self.out if d_out is None else d_out,
                                   gadget_label=self.ops["gadget_label"], **{key: self.d.get(key) for key in keys})

    def fetch(self):
        """-> ProveValues, as the host form returns it"""
        got = {}
        for key in self.names:
            raw = self.gpu.download(self.out[key], self.nb * self.per[key])
            if key in ("ok", "first_bad_row", "first_bad_gate"):
                size = self.per[key]
                raw = [int.from_bytes(raw[size * p:size * (p + 1)], "little", signed=True) for p in range(self.nb)]
            got[key] = raw
        got.setdefault("chi", None)
        got["planes"] = tuple(self.gpu.download(self.out[key], self.nb * self.per[key]) for key in ("a_L", "a_R", "a_O"))
        import mpc_bulletproof_amd as mm
        return mm.lib.ProveValues(**got)

    def free(self):
        for b in list(self.d.values()) + list(self.out.values()):
            self.gpu.free(b)


@pytest.mark.parametrize("nb", (1, 5))
@pytest.mark.parametrize("keys", (False, True), ids=("explicit", "keys"))
@pytest.mark.parametrize("name", NAMES)
def test_dev_form_equals_the_host_form(gpu, gens, made, name, keys, nb):
    """every operand and result on bpgpu_malloc buffers: after bpgpu_sync the bytes of the host form, on every output"""
    circ, w = made(name)
    ops = pc.operands(name, nb, keys)
    host = one_call(gpu, gens, circ, w, name, nb, ops)
    dev = Dev(gpu, name, nb, ops)
    try:
        dev.run(gens, circ, w)
        gpu.sync()
        got = dev.fetch()
        for field, a, b in zip(pc.FIELDS, got, host):
            assert a == b, field
        assert gpu.input_flag() == 0
        # the optional results left out
        dev.run(gens, circ, w, {key: dev.out[key] for key in ("ok", "points", "scalars")})
        assert gpu.download(dev.out["points"], nb * dev.per["points"]) == host.points and gpu.input_flag() == 0
    finally:
        dev.free()


@pytest.mark.parametrize("bad", (0, 2, 4), ids=("first", "middle", "last"))
@pytest.mark.parametrize("name", ("range8x2", "shuffle4"))
def test_dev_form_clears_a_rejected_provers_rows_without_waiting_for_ok(gpu, gens, made, name, bad):
    """the caller's bpgpu_malloc buffers, filled with 0xA5 beforehand: the call is enqueued and returns (nothing of it reads ok on
    the host), and after the sync the rejected prover's proof rows are zero bytes, the other provers' bytes are what they are
    without it, and the diagnostics are the chain's"""
    nb, keys = 5, True
    circ, w = made(name)
    ops = pc.operands(name, nb, keys, bad=bad)
    want = dict(zip(pc.FIELDS, pc.chain(gpu, gens, circ, w, name, nb, ops)))
    good = one_call(gpu, gens, circ, w, name, nb, pc.operands(name, nb, keys))
    dev = Dev(gpu, name, nb, ops)
    try:
        for key in PROOF_ROWS:
            gpu.upload(dev.out[key], b"\xa5" * (nb * dev.per[key]))
        dev.run(gens, circ, w)
        gpu.sync()
        got = dev.fetch()
        assert gpu.input_flag() == 0
    finally:
        dev.free()
    rest = [p for p in range(nb) if p != bad]
    assert got.ok == [int(p != bad) for p in range(nb)] == want["ok"]
    assert got.first_bad_row == want["first_bad_row"] and got.first_bad_gate == want["first_bad_gate"]
    assert (got.V, got.V_compressed, got.chi, got.planes) == (want["V"], want["V_compressed"], want["chi"], want["planes"])
    for field in PROOF_ROWS:
        data = getattr(got, field)
        assert pc.rows(name, field, data, [bad]) == bytes(pc.row_bytes(name)[field]), field
        assert pc.rows(name, field, data, rest) == pc.rows(name, field, getattr(good, field), rest) == pc.rows(name, field, want[field], rest), field
    assert verify(gpu, gens, circ, name, nb, got, ops) == got.ok


@pytest.mark.parametrize("name", ("range8x2", "composite"))
def test_a_non_canonical_limb(gpu, gens, made, name):
    """a committed value of prover 2 := the group order: the input flag in the `_dev` form, BPGPU_E_ARG in the host form, and the
    context is usable afterwards in both"""
    import mpc_bulletproof_amd as mm
    nb, keys = 5, True
    circ, w = made(name)
    m = pc.case(name).prog.m
    ops = pc.operands(name, nb, keys)
    host = one_call(gpu, gens, circ, w, name, nb, ops)
    bad = ops["v"][:32 * (2 * m + 1)] + N.to_bytes(32, "little") + ops["v"][32 * (2 * m + 2):]
    dev = Dev(gpu, name, nb, ops)
    try:
        gpu.upload(dev.d["v"], bad)
        dev.run(gens, circ, w)
        assert gpu.input_flag() == 1
        with pytest.raises(mm.BpGpuError) as e:
            one_call(gpu, gens, circ, w, name, nb, ops, v=bad)
        assert e.value.code == mm.lib.E_ARG
        gpu.upload(dev.d["v"], ops["v"])
        dev.run(gens, circ, w)
        assert gpu.input_flag() == 0 and dev.fetch() == host
        assert one_call(gpu, gens, circ, w, name, nb, ops) == host
    finally:
        dev.free()


_good = {}


@pytest.mark.parametrize("bad", (0, 2, 4), ids=("first", "middle", "last"))
@pytest.mark.parametrize("name", ("range8x2", "shuffle4"))
def test_a_rejected_prover_ships_nothing(gpu, gens, made, name, bad):
    """a range value of 2^8 with 8 bits | a shuffle whose outputs are no permutation of its inputs: ok 0, the chain's first_bad_row
    and V, every proof row zero bytes; the other four provers' bytes are what they are without it"""
    nb, keys = 5, False
    circ, w = made(name)
    ops = pc.operands(name, nb, keys, bad=bad)
    want = dict(zip(pc.FIELDS, pc.chain(gpu, gens, circ, w, name, nb, ops)))
    got = one_call(gpu, gens, circ, w, name, nb, ops)
    if name not in _good:
        _good[name] = one_call(gpu, gens, circ, w, name, nb, pc.operands(name, nb, keys))
    good = _good[name]
    rest = [p for p in range(nb) if p != bad]
    assert got.ok == [int(p != bad) for p in range(nb)] == want["ok"]
    assert got.first_bad_row == want["first_bad_row"] and got.first_bad_row[bad] >= 0
    assert got.first_bad_gate == want["first_bad_gate"] == [-1] * nb
    assert (got.V, got.V_compressed) == (want["V"], want["V_compressed"])
    assert got.planes == want["planes"] and got.chi == want["chi"]          # the diagnostics are left alone
    for field in PROOF_ROWS:
        data = getattr(got, field)
        assert pc.rows(name, field, data, [bad]) == bytes(pc.row_bytes(name)[field]), field
        assert pc.rows(name, field, data, rest) == pc.rows(name, field, getattr(good, field), rest) == pc.rows(name, field, want[field], rest), field
    assert pc.rows(name, "V", got.V, rest) == pc.rows(name, "V", good.V, rest)
    assert verify(gpu, gens, circ, name, nb, got, ops) == got.ok


def test_refusals_and_failures_leave_nothing_behind(gpu, gens, made):
    """every refusal on a live context, a launched call that fails on an operand, and then the next good call: the same bytes"""
    import mpc_bulletproof_amd as mm
    E = mm.lib
    for name in ("example", "composite"):
        circ, w = made(name)
        other_circ, other_w = made("shuffle4" if name == "composite" else "range8x2")
        prog = pc.case(name).prog
        ops = pc.operands(name, 1, False)
        before = one_call(gpu, gens, circ, w, name, 1, ops)
        small = gpu.gens_create(o.gens("G", 4), o.gens("H", 4), o.generator(), o.generator(), 8)

        def code(g=gens, c=circ, prog_=w, **over):
            try:
                gpu.r1cs_prove_values(g, c, prog_, 1, prog.n, prog.m, **dict(ops, **over))
            except E.BpGpuError as e:
                return e.code
            return 0
        try:
            assert code(prog_=other_w) == E.E_ARG and code(c=other_circ) == E.E_ARG         # not the circuit's program
            assert code(prog_=None) == E.E_ARG and code(c=None) == E.E_ARG and code(g=None) == E.E_ARG
            for key in ("init_states", "v", "v_blinding", "blindings") + (("inputs",) if prog.ninp else ()):
                assert code(**{key: None}) == E.E_ARG, key
            assert code(gadget_label=None if pc.two_phase(name) else pc.LABEL) == E.E_ARG      # the label and the shape disagree
            assert code(s_L=None) == E.E_ARG and code(s_L=None, s_R=None) == E.E_ARG and code(vector_keys=bytes(64)) == E.E_ARG
            if prog.n > 4:
                assert code(g=small) == E.E_GENS
            gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, 0, 2))
            try:
                assert code() == E.E_ARG
            finally:
                gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, 0, 1))
            # launched calls that fail on an operand
            assert code(v=N.to_bytes(32, "little") + ops["v"][32:]) == E.E_ARG
            assert code(blindings=ops["blindings"][:-32] + N.to_bytes(32, "little")) == E.E_ARG
            assert E._lib.bpgpu_r1cs_prove_values(gpu.ctx, gens, circ, w, 0, *([None] * 23)) == 0          # nb == 0
            assert one_call(gpu, gens, circ, w, name, 1, ops) == before
        finally:
            gpu.gens_destroy(small)
