"""BPGPU_GATE_DIVREM (include/bpgpu.h) on the CPU: the op's value in the binding and the header; bpgpu_witness_create accepts a program
with a DIVREM gate past its refusals and refuses ops 3, 5, 7 and 255, a chi part in phase 1 and a self reference, all before a device
is touched; bpgpu_witness_plan / _gate_levels / _chains / _affine_chains against the helper's own levels and chains on every case of
tests/witness_divrem_cases.py; and bpgpu_mpc_witness_begin refuses a phase that holds a DIVREM gate.  No GPU needed."""
import ctypes as C
import os

import witness_affine_cases as af
import witness_cases as wc
import witness_chain_cases as cc
import witness_divrem_cases as dc

N = wc.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, R, O, V, ONE = wc.L, wc.R, wc.O, wc.V, wc.ONE
NBS = (1, 65)
READ_AS_MUL_DIFFERS = ("dr_rows",)        # there the MUL reading would make the link-shaped DIVREM gate a chain member


def _lib():
    import mpc_bulletproof_amd as m
    return m, m.lib._lib


def test_the_op_is_6_in_the_binding_and_the_header():
    m, _ = _lib()
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    assert m.lib.GATE_DIVREM == 6 == dc.DIVREM
    assert "#define BPGPU_GATE_DIVREM 6" in hdr and "#define BPGPU_GATE_DIVREM 5" not in hdr and "#define BPGPU_GATE_INV 4" in hdr
    flat = " ".join(hdr.replace("*", " ").split())
    assert "BPGPU_GATE_DIVREM the integer quotient and remainder" in flat            # the op's paragraph
    assert "a_L[i] = floor(x / y), a_R[i] = x mod y" in flat and "a_L[i] = 0 and a_R[i] = x" in flat
    assert "BPGPU_GATE_DIVREM gate in the evaluated phase" in flat                   # the refusal on shares, in the two-party block
    assert "not 5:" in flat


def _create(lib, prog=None, **over):
    u32 = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs)      # noqa: E731
    n, n1, m, nchi, op, arg, rp, kd, ix, cf = prog.create_args()
    a = dict(n=n, n1=n1, m=m, nchi=nchi, op=op, arg=arg, rp=rp, kd=kd, ix=ix, cf=cf)
    a.update(over)
    fake_ctx = (C.c_uint8 * (1 << 16))()
    h = C.c_void_p()
    rc = lib.bpgpu_witness_create(fake_ctx, a["n"], a["n1"], a["m"], a["nchi"], bytes(a["op"]), u32(a["arg"]), u32(a["rp"]), u32(a["kd"]),
                                  u32(a["ix"]), a["cf"], C.byref(h))
    assert not h.value or rc == 0
    return rc


def _small():
    """gate 0 = divrem(v_0 + 1, v_1), gate 1 = multiply(a_L[0], a_R[0])"""
    prog = dc.Program(2)
    prog.divrem([(V, 0, 1), (ONE, 0, 1)], [(V, 1, 1)])
    prog.mul([(L, 0, 1)], [(R, 0, 1)])
    prog.end_phase1()
    return prog


def test_a_valid_divrem_program_passes_the_refusals_of_witness_create():
    """past the refusals the first thing the call does is select the context's device: over a zeroed context that fails with
    BPGPU_E_DEVICE where there is none (and with a device, tests/test_gpu_witness_divrem.py creates the programs for real).  Before
    the op existed the answer was BPGPU_E_ARG: an unknown op"""
    m, lib = _lib()
    rc = _create(lib, _small())
    assert rc != m.lib.E_ARG
    if lib.bpgpu_device_count() == 0:
        assert rc == m.lib.E_DEVICE
        for c in dc.cases():
            assert _create(lib, c.prog) == m.lib.E_DEVICE, c.name


def test_witness_create_refusals_around_the_op():
    m, lib = _lib()
    E = m.lib.E_ARG
    prog = _small()
    for op in (3, 5, 7, 255):
        assert _create(lib, prog, op=[op, 0]) == E, op                   # no ops, below and above 6
        assert _create(lib, prog, op=[6, op]) == E, op
    # the validation of a MUL gate with the same rows
    chi1 = dc.Program(1, nchi=1)
    chi1.divrem([(V, 0, 1)], [(V, 0, (None, 1))])
    chi1.end_phase1()
    assert _create(lib, chi1) == E                                       # a chi part in phase 1
    chi2 = dc.Program(1, nchi=1)
    chi2.end_phase1()
    chi2.divrem([(V, 0, 1)], [(V, 0, (None, 1))])
    assert _create(lib, chi2) != E                                       # ... the same gate in phase 2 is fine
    for row in ([(O, 0, 1)], [(L, 1, 1)]):
        ref = dc.Program(1)
        ref.divrem([(V, 0, 1)], row)
        ref.end_phase1()
        assert _create(lib, ref) == E                                    # a self and a forward reference
    beyond = dc.Program(1)
    beyond.divrem([(V, 1, 1)], [])
    beyond.end_phase1()
    assert _create(lib, beyond) == E                                     # a committed index >= m
    empty = dc.Program(1)
    empty.divrem([], [])
    empty.end_phase1()
    assert _create(lib, empty) != E                                      # both rows may be empty: 0 / 0
    assert _create(lib, prog, arg=[252, 7]) == _create(lib, prog)        # arg is ignored


def _levels(prog):
    level = []
    for i, (op, _, left, right) in enumerate(prog.gates):
        lo = 0 if i < prog.phase1 else prog.phase1
        reads = [idx for kind, idx, _ in left + right if kind <= O and idx >= lo]
        level.append(0 if op == wc.INPUT or not reads else 1 + max(level[r] for r in reads))
    return level


def test_plan_levels_and_chains_equal_the_helpers_on_every_case():
    import mpc_bulletproof_amd as m
    for case in dc.cases():
        prog = case.prog
        n, n1, nchi, ops, rp, kd, ix = prog.plan_args()
        as_mul = [wc.MUL if op == dc.DIVREM else op for op in ops]
        for nb in NBS:
            plan = m.lib.witness_plan(*prog.plan_args(), nb)
            l1, l2, widest, long_rows = prog.levels()
            assert (plan["levels1"], plan["levels2"], plan["widest"], plan["long_rows"], plan["inputs"]) == (l1, l2, widest, long_rows, 0), case.name
            # the route rule is unchanged: the plan of the program with every DIVREM gate read as a MUL gate
            if case.name not in READ_AS_MUL_DIFFERS:
                assert plan == m.lib.witness_plan(n, n1, nchi, as_mul, rp, kd, ix, nb), case.name
                assert m.lib.witness_chains(*prog.plan_args()) == m.lib.witness_chains(n, n1, nchi, as_mul, rp, kd, ix), case.name
        assert m.lib.witness_chains(*prog.plan_args()) == cc.figures(prog), case.name
        assert m.lib.witness_affine_chains(*prog.plan_args()) == af.figures(prog), case.name
        assert list(m.lib.witness_gate_levels(*prog.plan_args()))[:prog.n] == _levels(prog), case.name


def test_chains_around_divrem_gates():
    import mpc_bulletproof_amd as m
    prog = dc.case("dr_head").prog
    pred, _, figs = cc.analyse(prog)
    head, aff_head = 0, prog.affine_head
    assert prog.gates[head][0] == dc.DIVREM and prog.gates[aff_head][0] == dc.DIVREM
    # the DIVREM gate heads the chain of HEAD_MEMBERS MUL members, the first of which links to its a_O
    assert pred[head] is None and pred[1] == head and figs["longest"][0] == dc.HEAD_MEMBERS
    got = m.lib.witness_chains(*prog.plan_args())
    assert (got["chains1"], got["members1"], got["longest1"]) == (1, dc.HEAD_MEMBERS, dc.HEAD_MEMBERS)
    aff = m.lib.witness_affine_chains(*prog.plan_args())
    assert (aff["chains1"], aff["affine1"], aff["longest1"], aff["levels1"]) == (2, dc.AFFINE_MEMBERS, dc.HEAD_MEMBERS, 1)
    # a DIVREM gate whose rows have the link shape stays ordinary: one level above the gate it reads, no member anywhere
    rows = dc.case("dr_rows").prog
    got = m.lib.witness_chains(*rows.plan_args())
    assert (got["chains1"], got["members1"]) == (0, 0) and _levels(rows)[rows.link_shaped] == 1
    n, n1, nchi, ops, rp, kd, ix = rows.plan_args()
    as_mul = [wc.MUL if op == dc.DIVREM else op for op in ops]
    assert m.lib.witness_chains(n, n1, nchi, as_mul, rp, kd, ix)["members1"] >= 1


def test_mpc_witness_begin_refuses_a_phase_with_a_divrem_gate():
    """hand-made headers for the handle (its leading fields: n n1 m nchi inputs | BIT gates per phase | INV gates per phase | DIVREM
    gates per phase): the refusal comes before a device is touched, like the ones for BIT and INV gates"""
    m, lib = _lib()
    E = m.lib.E_ARG
    fake_ctx = (C.c_uint8 * (1 << 16))()
    buf = (C.c_uint8 * 4096)()

    def prog(div1=0, div2=0):
        return (C.c_size_t * 64)(2, 1, 1, 0, 0, 0, 0, div1 | div2 << 32)

    def begin(w, phase):
        h = C.c_void_p()
        rc = lib.bpgpu_mpc_witness_begin(fake_ctx, w, 1, phase, buf, None, None, buf, buf, buf, C.byref(h))
        assert not h.value
        return rc
    past = m.lib.E_DEVICE if lib.bpgpu_device_count() == 0 else None
    for phase in (0, 1, 2):
        rc = begin(prog(), phase)
        assert rc != E and (past is None or rc == past), phase
    assert begin(prog(div1=1), 0) == E and begin(prog(div1=1), 1) == E
    assert begin(prog(div2=1), 0) == E and begin(prog(div2=1), 2) == E
    # phase 1 of a program whose DIVREM gates are all in phase 2 is evaluated as before, and the other way round
    for w, phase in ((prog(div2=3), 1), (prog(div1=3), 2)):
        rc = begin(w, phase)
        assert rc != E and (past is None or rc == past), phase


def test_phases_compose_on_every_case():
    for case in dc.cases():
        for p in range(len(case.provers)):
            v, inputs, chi = case.prover(p)
            first = case.prog.evaluate(v, inputs, chi, phase=1)
            assert tuple(case.prog.evaluate(v, inputs, chi, phase=2, planes=first)) == tuple(case.want(p)), case.name
