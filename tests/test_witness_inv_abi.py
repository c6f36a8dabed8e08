"""BPGPU_GATE_INV (include/bpgpu.h) on the CPU: the op's value in the binding and the header; bpgpu_witness_create accepts a program
with an INV gate past its refusals and refuses a non-empty right row, ops 3 and 5 and a chi part in phase 1, all before a device is
touched; bpgpu_witness_plan / _gate_levels / _chains / _affine_chains against the helper's own levels and chains on every case of
tests/witness_inv_cases.py; bpgpu_mpc_witness_begin refuses a phase that holds an INV gate; and a self-check of the cases
tests/test_gpu_witness_inv.py runs on the GPU.  No GPU needed."""
import ctypes as C
import os

import witness_affine_cases as af
import witness_cases as wc
import witness_chain_cases as cc
import witness_inv_cases as ic

N = wc.N
pm = wc.pm
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import mpc_bulletproof_amd as m
    return m, m.lib._lib


def test_the_op_is_4_in_the_binding_and_the_header():
    m, _ = _lib()
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    assert m.lib.GATE_INV == 4 == ic.INV
    assert "#define BPGPU_GATE_INV 4" in hdr and "#define BPGPU_GATE_INV 3" not in hdr
    assert "#define BPGPU_WIT_PLAN_FIELDS 7" in hdr and "#define BPGPU_OPT_COUNT 22" in hdr
    flat = " ".join(hdr.replace("*", " ").split())
    assert "BPGPU_GATE_INV gate in the evaluated phase" in flat          # the refusal on shares, in the two-party block


def _create(lib, prog=None, **over):
    u32 = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs)      # noqa: E731
    n, n1, m, nchi, op, arg, rp, kd, ix, cf = prog.create_args() if prog is not None else (None,) * 10
    a = dict(n=n, n1=n1, m=m, nchi=nchi, op=op, arg=arg, rp=rp, kd=kd, ix=ix, cf=cf)
    a.update(over)
    fake_ctx = (C.c_uint8 * (1 << 16))()
    h = C.c_void_p()
    rc = lib.bpgpu_witness_create(fake_ctx, a["n"], a["n1"], a["m"], a["nchi"], bytes(a["op"]), u32(a["arg"]), u32(a["rp"]), u32(a["kd"]),
                                  u32(a["ix"]), a["cf"], C.byref(h))
    assert not h.value or rc == 0
    return rc


def _small(nchi=0, phase1=True):
    """gate 0 = inv(v_0 + 1), gate 1 = multiply(a_O[0], a_R[0])"""
    prog = ic.Program(1, nchi)
    if not phase1:
        prog.end_phase1()
    prog.inv([(V, 0, 1), (ONE, 0, 1)])
    prog.mul([(O, 0, 1)], [(R, 0, 1)])
    if phase1:
        prog.end_phase1()
    return prog


V, ONE, O, R = wc.V, wc.ONE, wc.O, wc.R


def test_a_valid_inv_program_passes_the_refusals_of_witness_create():
    """past the refusals the first thing the call does is select the context's device: over a zeroed context that fails with
    BPGPU_E_DEVICE where there is none (and with a device, tests/test_gpu_witness_inv.py creates the programs for real).  Before
    the op existed the answer was BPGPU_E_ARG: an unknown op"""
    m, lib = _lib()
    rc = _create(lib, _small())
    assert rc != m.lib.E_ARG
    if lib.bpgpu_device_count() == 0:
        assert rc == m.lib.E_DEVICE
        for c in ic.cases():
            assert _create(lib, c.prog) == m.lib.E_DEVICE, c.name


def test_witness_create_refusals_of_the_op():
    m, lib = _lib()
    E = m.lib.E_ARG
    prog = _small()
    with_right = ic.Program(1)
    with_right._add(ic.INV, 0, [(V, 0, 1)], [(ONE, 0, 1)])
    with_right.end_phase1()
    assert _create(lib, with_right) == E                                 # an INV gate with a non-empty right row
    assert _create(lib, prog, op=[3, 0]) == E                            # 3 is no op
    assert _create(lib, prog, op=[5, 0]) == E and _create(lib, prog, op=[255, 0]) == E
    chi1 = ic.Program(1, nchi=1)
    chi1.inv([(V, 0, (None, 1))])
    chi1.end_phase1()
    assert _create(lib, chi1) == E                                       # a chi part in phase 1
    chi2 = ic.Program(1, nchi=1)
    chi2.end_phase1()
    chi2.inv([(V, 0, (None, 1))])
    assert _create(lib, chi2) != E                                       # ... the same gate in phase 2 is fine
    self_ref = ic.Program(1)
    self_ref.inv([(O, 0, 1)])
    self_ref.end_phase1()
    assert _create(lib, self_ref) == E                                   # a self reference
    # arg is ignored
    assert _create(lib, prog, arg=[252, 7]) == _create(lib, prog)


def test_plan_levels_and_chains_equal_the_helpers_on_every_case():
    import mpc_bulletproof_amd as m
    for case in ic.cases():
        prog = case.prog
        for nb in (1, 65):
            plan = m.lib.witness_plan(*prog.plan_args(), nb)
            l1, l2, widest, long_rows = prog.levels()
            assert (plan["levels1"], plan["levels2"], plan["widest"], plan["long_rows"], plan["inputs"]) == (l1, l2, widest, long_rows, 0), case.name
            # the route rule is unchanged: the plan of the program with every INV gate read as a MUL gate
            as_mul = [wc.MUL if op == ic.INV else op for op in prog.ops()]
            n, n1, nchi, _, rp, kd, ix = prog.plan_args()
            if case.name not in ("inv_head",):                           # (there the MUL reading would make the INV gate a member)
                assert plan == m.lib.witness_plan(n, n1, nchi, as_mul, rp, kd, ix, nb), case.name
        assert m.lib.witness_chains(*prog.plan_args()) == cc.figures(prog), case.name
        assert m.lib.witness_affine_chains(*prog.plan_args()) == af.figures(prog), case.name
        assert list(m.lib.witness_gate_levels(*prog.plan_args()))[:prog.n] == _levels(prog), case.name


def _levels(prog):
    level = []
    for i, (op, _, left, right) in enumerate(prog.gates):
        lo = 0 if i < prog.phase1 else prog.phase1
        reads = [idx for kind, idx, _ in left + right if kind <= O and idx >= lo]
        level.append(0 if op == wc.INPUT or not reads else 1 + max(level[r] for r in reads))
    return level


def test_chains_around_inv_gates():
    import mpc_bulletproof_amd as m
    prog = ic.case("inv_head").prog
    pred, right, figs = cc.analyse(prog)
    head, stays = 0, ic.HEAD_MEMBERS + 2
    assert prog.gates[head][0] == ic.INV and prog.gates[stays][0] == ic.INV
    # the INV gate heads the chain of HEAD_MEMBERS members
    assert pred[head] is None and pred[1] == head and figs["longest"][0] == ic.HEAD_MEMBERS
    # an INV gate whose row is one a_O term of its phase stays ordinary; the MUL after it takes the link it left free
    assert pred[stays] is None and pred[stays + 1] == stays - 1
    # ... and a MUL member links to the INV gate's a_O
    assert pred[stays + 2] == stays
    got = m.lib.witness_chains(*prog.plan_args())
    assert (got["chains1"], got["members1"], got["longest1"]) == (3, ic.HEAD_MEMBERS + 2, ic.HEAD_MEMBERS)
    assert _levels(prog)[stays] == 1 and got["levels1"] == 2
    # the affine chain on an INV gate's a_O
    aff = m.lib.witness_affine_chains(*ic.case("inv_affine").prog.plan_args())
    assert (aff["chains1"], aff["affine1"], aff["longest1"], aff["levels1"]) == (1, ic.AFFINE_MEMBERS, ic.AFFINE_MEMBERS, 1)
    # the INV chain: one gate per level, nothing compressed
    deep = ic.case("inv_deep").prog
    assert m.lib.witness_plan(*deep.plan_args(), 1)["levels1"] == ic.DEPTH + 3 == m.lib.witness_affine_chains(*deep.plan_args())["levels1"]


def test_mpc_witness_begin_refuses_a_phase_with_an_inv_gate():
    """hand-made headers for the handle (its leading fields: n n1 m nchi inputs | BIT gates per phase | INV gates per phase): the
    refusal comes before a device is touched, like the one for BIT gates"""
    m, lib = _lib()
    E = m.lib.E_ARG
    fake_ctx = (C.c_uint8 * (1 << 16))()
    buf = (C.c_uint8 * 4096)()

    def prog(inv1=0, inv2=0):
        return (C.c_size_t * 64)(2, 1, 1, 0, 0, 0, inv1 | inv2 << 32)

    def begin(w, phase):
        h = C.c_void_p()
        rc = lib.bpgpu_mpc_witness_begin(fake_ctx, w, 1, phase, buf, None, None, buf, buf, buf, C.byref(h))
        assert not h.value
        return rc
    past = m.lib.E_DEVICE if lib.bpgpu_device_count() == 0 else None
    for phase in (0, 1, 2):
        rc = begin(prog(), phase)
        assert rc != E and (past is None or rc == past), phase
    assert begin(prog(inv1=1), 0) == E and begin(prog(inv1=1), 1) == E
    assert begin(prog(inv2=1), 0) == E and begin(prog(inv2=1), 2) == E
    # phase 1 of a program whose INV gates are all in phase 2 is evaluated as before, and the other way round
    for w, phase in ((prog(inv2=3), 1), (prog(inv1=3), 2)):
        rc = begin(w, phase)
        assert rc != E and (past is None or rc == past), phase


def test_evaluator_reproduces_the_model_provers_witness_and_it_satisfies_the_circuit():
    for case in ic.gadget_cases():
        for p in range(len(case.provers)):
            pv = case.model(p)
            assert (pv.a_L, pv.a_R, pv.a_O) == tuple(case.want(p)), (case.name, p)
            assert all(pv.eval(lc) == 0 for lc in pv.constraints), (case.name, p)
            assert all(l * r % N == o for l, r, o in zip(pv.a_L, pv.a_R, pv.a_O))
            assert len(pv.a_L) == case.prog.n
            for i, (op, _, _, _) in enumerate(case.prog.gates):
                if op == ic.INV:
                    assert pv.a_O[i] == int(pv.a_L[i] != 0) and pv.a_R[i] == ic.inv_or_zero(pv.a_L[i])


def test_parametric_circuit_of_a_case_serves_every_prover_of_it():
    for case in ic.gadget_cases():
        q, nchi, rp, kd, ix, cf = wc.circuit_csr(case)
        coeff = [int.from_bytes(cf[32 * t:32 * t + 32], "little") for t in range(len(kd))]
        for p in range(len(case.provers)):
            v, _, chi = case.prover(p)
            planes = tuple(case.want(p)) + (v,)
            for r in range(q):
                tot = 0
                for j in range(1 + nchi):
                    for t in range(rp[j * q + r], rp[j * q + r + 1]):
                        tot += coeff[t] * (chi[j - 1] if j else 1) * (1 if kd[t] == 4 else planes[kd[t]][ix[t]])
                assert tot % N == 0, (case.name, p, r)


def test_a_false_claim_and_a_wrong_inverse_do_not_satisfy_the_circuit():
    for case in ic.gadget_cases():
        v, inputs, chi = case.prover(0)
        v2, inputs2 = case.breaker(v, inputs)
        broken = wc.Case(case.name, case.prog, [(v2, inputs2, chi)], case.gadget)
        pv = broken.model(0)
        assert (pv.a_L, pv.a_R, pv.a_O) == tuple(broken.want(0)), case.name       # still the gadget's witness ...
        assert any(pv.eval(lc) for lc in pv.constraints), case.name               # ... of a claim that does not hold
    case = ic.case("inv_is_zero")
    wrong = wc.Case(case.name, case.prog, case.provers, lambda cs, var, v, inputs: case.gadget(cs, var, v, inputs, wrong_inverse=True))
    pv = wrong.model(0)
    assert (pv.a_L, pv.a_R, pv.a_O) != tuple(case.want(0))
    assert any(pv.eval(lc) for lc in pv.constraints)


def test_phases_compose_and_the_cases_cover_what_they_claim():
    for case in ic.cases():
        for p in range(len(case.provers)):
            v, inputs, chi = case.prover(p)
            first = case.prog.evaluate(v, inputs, chi, phase=1)
            assert tuple(case.prog.evaluate(v, inputs, chi, phase=2, planes=first)) == tuple(case.want(p)), case.name
    for size in ic.LEVEL_SIZES:
        case = ic.case("inv_level%d" % size)
        zeros = [{i for i in range(size) if pr[0][i] == 0} for pr in case.provers]
        assert set() in zeros and {0} in zeros and {size - 1} in zeros and set(range(size)) in zeros and set(range(0, size, 256)) in zeros
        assert all({i} in zeros for i in range(0, size, 256))
        assert case.prog.levels()[2] == size
    assert ic.case("inv_long").prog.levels()[3] == 3
    chi_zero = ic.case("inv_chi")
    n1 = chi_zero.prog.phase1
    assert [chi_zero.want(p)[0][n1] == 0 for p in range(3)] == [True, False, False] and chi_zero.want(2)[0][n1 + 2] == 0
    edges = ic.case("inv_edges")
    assert {x for x in edges.want(0)[0]} >= set(wc.EDGE)
    two = ic.case("inv_two_phase").prog
    assert any(g[0] == ic.INV for g in two.gates[:two.phase1]) and two.gates[-1][0] == ic.INV
