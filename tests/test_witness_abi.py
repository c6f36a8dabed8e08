"""The witness-synthesis entry points of include/bpgpu.h on the CPU: exported, bound and declared for Rust with the header's argument
counts; every refusal of bpgpu_witness_create, bpgpu_r1cs_witness_synthesize and bpgpu_r1cs_prove_fs2 comes back before a device is
touched; bpgpu_witness_plan against the helper's own levels; and a self-check of the cases that tests/test_gpu_witness.py runs on the
GPU: the helper's evaluator reproduces the model prover's witness, which satisfies its circuit.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

import witness_cases as wc

N = wc.N
pm = wc.pm
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of arguments
NEW = {"bpgpu_witness_create": 12, "bpgpu_witness_destroy": 2, "bpgpu_witness_plan": 9,
       "bpgpu_r1cs_witness_synthesize": 10, "bpgpu_r1cs_witness_synthesize_dev": 10,
       "bpgpu_r1cs_prove_fs2": 23, "bpgpu_r1cs_prove_fs2_dev": 23}


def _lib():
    import mpc_bulletproof_amd as m
    return m, m.lib._lib


def test_entry_points_are_exported_bound_and_declared_with_their_argument_counts():
    m, lib = _lib()
    from mpc_bulletproof_amd._abi import PROTOS
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert name in m.lib.SYMBOLS, name
        decl = re.search(r"\b(?:int|void) %s\s*\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        rdecl = re.search(r"pub fn %s\(([^;]*)\)\s*(?:->|;)" % name, rs, re.S)
        assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == nargs, name
        assert len(PROTOS[name][1]) == nargs and getattr(lib, name).argtypes == PROTOS[name][1], name
        assert callable(getattr(m.BpGpu, name[len("bpgpu_"):])), name
    assert "pub struct bpgpu_witness" in rs
    assert m.lib.OPT["witness_route"] == 20 and "#define BPGPU_OPT_WITNESS_ROUTE 20" in hdr
    assert "#define BPGPU_PROF_KINDS 24" in hdr
    assert (m.lib.GATE_MUL, m.lib.GATE_INPUT, m.lib.GATE_BIT) == (0, 1, 2) == (wc.MUL, wc.INPUT, wc.BIT)


def test_header_no_longer_calls_the_round_trip_inherent_for_every_gadget():
    hdr = " ".join(open(os.path.join(ROOT, "include", "bpgpu.h")).read().replace("*", " ").split())
    assert "so that round trip is inherent" not in hdr and "that is the only round trip left" not in hdr
    assert "inherent only to a gadget that no bpgpu_witness gate program describes" in hdr
    block = hdr[hdr.index("witness synthesis: Prover::multiply"):hdr.index("int bpgpu_r1cs_prove_fs2_dev(")]
    for phrase in ("BPGPU_GATE_MUL", "BPGPU_GATE_INPUT", "BPGPU_GATE_BIT", "arg[i] < 252", "a self or forward reference", "sorted by level",
                   "UNMEASURED", "bpgpu_input_flag", "nb == 0: BPGPU_OK", "leaves no pool memory behind", "kind 22", "host mirror", "Beaver step",
                   "bench.py", "i1 o1 s1 | i2 o2 s2 tb1 tb3 tb4 tb5 tb6", "nb x 2 x 32", "no session left behind"):
        assert phrase in block, phrase


# ---- bpgpu_witness_create: every refusal, before a device is touched (a zeroed block stands in for the context)
def _create(lib, n, n1, m, nchi, op, arg, rp, kd, ix, cf, ctx="fake", out="out"):
    u32 = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs) if xs is not None else None     # noqa: E731
    fake_ctx = (C.c_uint8 * (1 << 16))()
    h = C.c_void_p()
    rc = lib.bpgpu_witness_create(fake_ctx if ctx == "fake" else ctx, n, n1, m, nchi, bytes(op) if op is not None else None, u32(arg), u32(rp),
                                  u32(kd), u32(ix), cf, C.byref(h) if out == "out" else out)
    assert not h.value or rc == 0
    return rc


def _one(c):
    return wc.le(c)


def test_witness_create_refusals_come_back_without_a_device():
    m, lib = _lib()
    E, EL = m.lib.E_ARG, m.lib.E_LEN
    # a valid two-gate program: gate 0 = multiply(v_0, 1), gate 1 = multiply(a_O[0], v_1)
    op, arg = [0, 0], [0, 0]
    rp, kd, ix = [0, 1, 2, 3, 4], [3, 4, 2, 3], [0, 0, 0, 1]
    cf = b"".join(_one(1) for _ in range(4))
    good = dict(n=2, n1=2, m=2, nchi=0, op=op, arg=arg, rp=rp, kd=kd, ix=ix, cf=cf)

    def rc(**kw):
        return _create(lib, **dict(good, **kw))

    def passes(**kw):
        """past the refusals the first thing a call does is select the context's device: without one, that is what it reports (with one,
        tests/test_gpu_witness.py creates the valid programs on a real context)"""
        if lib.bpgpu_device_count() == 0:
            assert rc(**kw) == m.lib.E_DEVICE, kw
    passes()
    assert rc(ctx=None) == E and rc(out=None) == E           # null pointers
    for hole in ("op", "arg", "rp", "kd", "ix", "cf"):
        assert rc(**{hole: None}) == E, hole
    assert rc(op=[0, 3]) == E                                # an unknown op
    assert rc(kd=[3, 4, 5, 3]) == E                          # ... and kind
    assert rc(ix=[0, 0, 1, 1]) == E                          # gate 1 reads its own a_O: a self reference
    assert rc(ix=[0, 0, 0, 1], kd=[0, 4, 2, 3]) == E         # gate 0 reads a_L[0]
    assert rc(kd=[3, 4, 1, 3], ix=[0, 0, 7, 1]) == E         # a forward reference
    assert rc(ix=[2, 0, 0, 1]) == E                          # a committed index >= m
    assert rc(ix=[0, 0, 0, 2]) == E
    assert rc(n1=3) == E                                     # n1 > n
    assert rc(nchi=9, rp=[0, 1, 2, 3, 4] + [4] * 36) == E    # nchi > 8
    assert rc(rp=[0, 2, 1, 3, 4]) == E                       # row pointers that decrease
    assert rc(cf=_one(1) * 3 + N.to_bytes(32, "little")) == E      # a non-canonical coefficient
    # a chi part in a gate < n1: the challenge does not exist in phase 1 (the same part is fine in phase 2)
    chi_rp = [0, 1, 2, 3, 4, 4, 5, 5, 5]
    chi_kd, chi_ix, chi_cf = kd + [4], ix + [0], cf + _one(N - 1)
    assert rc(nchi=1, rp=chi_rp, kd=chi_kd, ix=chi_ix, cf=chi_cf) == E
    passes(nchi=1, n1=1, rp=[0, 1, 2, 3, 4, 4, 4, 4, 5], kd=chi_kd, ix=chi_ix, cf=chi_cf)
    assert rc(nchi=1, n1=1, rp=chi_rp, kd=chi_kd, ix=chi_ix, cf=chi_cf) == E
    # BIT: arg < 252, an empty right row
    assert rc(op=[2, 0], arg=[252, 0], rp=[0, 1, 1, 2, 3], kd=[3, 2, 3], ix=[0, 0, 1], cf=cf[:96]) == E
    assert rc(op=[2, 0], arg=[251, 0]) == E                  # (its right row holds the constant)
    passes(op=[2, 0], arg=[251, 0], rp=[0, 1, 1, 2, 3], kd=[3, 2, 3], ix=[0, 0, 1], cf=cf[:96])
    # INPUT: both rows empty
    assert rc(op=[1, 0]) == E
    assert rc(op=[1, 0], rp=[0, 0, 1, 2, 3], kd=[4, 2, 3], ix=[0, 0, 1], cf=cf[:96]) == E
    passes(op=[1, 0], rp=[0, 0, 0, 1, 2], kd=[2, 3], ix=[0, 1], cf=cf[:64])
    # n or m above 2^25 - 1 (nothing of the arrays is read past the counts' check)
    assert rc(m=1 << 25) == EL
    assert lib.bpgpu_witness_create((C.c_uint8 * 64)(), 1 << 25, 0, 0, 0, bytes(1), (C.c_uint32 * 1)(), (C.c_uint32 * 1)(), None, None, None,
                                    C.byref(C.c_void_p())) == EL


# ---- bpgpu_r1cs_witness_synthesize / bpgpu_r1cs_prove_fs2: hand-made headers for the handles (their leading fields)
def test_synthesize_refusals_come_back_without_a_device():
    m, lib = _lib()
    E = m.lib.E_ARG
    fake_ctx = (C.c_uint8 * (1 << 16))()
    numeric = (C.c_size_t * 64)(2, 2, 1, 0, 1)           # n, n1, m, nchi, INPUT pairs
    param = (C.c_size_t * 64)(2, 1, 1, 1, 0)
    bare = (C.c_size_t * 64)(0, 0, 0, 0, 0)
    buf = (C.c_uint8 * 4096)()
    for name in ("bpgpu_r1cs_witness_synthesize", "bpgpu_r1cs_witness_synthesize_dev"):
        call = lambda ctx, w, nb, phase, v, inp, chi, aL, aR, aO: getattr(lib, name)(ctx, w, nb, phase, v, inp, chi, aL, aR, aO)   # noqa: E731
        assert call(None, numeric, 1, 0, buf, buf, None, buf, buf, buf) == E, name               # no context
        assert call(fake_ctx, None, 1, 0, buf, buf, None, buf, buf, buf) == E, name              # no program
        for phase in (-1, 3):
            assert call(fake_ctx, numeric, 1, phase, buf, buf, None, buf, buf, buf) == E, name   # a bad phase
            assert call(fake_ctx, numeric, 0, phase, buf, buf, None, buf, buf, buf) == E, name
        for hole in (0, 1, 3, 4, 5):                                                             # v, inputs, a_L, a_R, a_O
            ops = [buf, buf, None, buf, buf, buf]
            ops[hole] = None
            assert call(fake_ctx, numeric, 1, 0, *ops) == E, (name, hole)
        assert call(fake_ctx, numeric, 1, 0, buf, buf, buf, buf, buf, buf) == E, name            # challenges for a numeric program
        for phase in (0, 2):
            assert call(fake_ctx, param, 1, phase, buf, None, None, buf, buf, buf) == E, name    # none for a parametric one's phase 2
        assert call(fake_ctx, param, 1, 1, buf, None, buf, buf, buf, buf) == E, name             # ... and given where phase 1 runs alone
        assert call(fake_ctx, numeric, 0, 0, None, None, None, None, None, None) == 0, name      # nb == 0: nothing to do
        assert call(fake_ctx, param, 0, 2, None, None, buf, None, None, None) == 0, name
        if lib.bpgpu_device_count() == 0:
            assert call(fake_ctx, numeric, 1, 0, buf, buf, None, buf, buf, buf) == m.lib.E_DEVICE, name
            assert call(fake_ctx, param, 1, 1, buf, None, None, buf, buf, buf) == m.lib.E_DEVICE, name
            assert call(fake_ctx, bare, 1, 0, None, None, None, None, None, None) == m.lib.E_DEVICE, name


def test_prove_fs2_refusals_come_back_without_a_device():
    m, lib = _lib()
    E = m.lib.E_ARG
    fake_ctx = (C.c_uint8 * (1 << 16))()
    gens = (C.c_size_t * 64)(4)                          # capacity
    circ = (C.c_size_t * 64)(5, 3, 2, 7, 1)              # q, n, m, nnz, nchi
    numeric = (C.c_size_t * 64)(5, 3, 2, 7, 0)
    two_chi = (C.c_size_t * 64)(5, 3, 2, 7, 2)
    prog = (C.c_size_t * 64)(3, 1, 2, 1, 1)              # n, n1, m, nchi, INPUT pairs
    buf = (C.c_uint8 * 4096)()
    # ctx g c w nb | states label v inputs s_L s_R keys v_blinding blindings | points scalars wire ch states chi | a_L a_R a_O
    good = [fake_ctx, gens, circ, prog, 1, buf, buf, buf, buf, buf, buf, None, buf, buf, buf, buf, None, None, None, None, None, None, None]
    for name in ("bpgpu_r1cs_prove_fs2", "bpgpu_r1cs_prove_fs2_dev"):
        fn = getattr(lib, name)

        def rc(**kw):
            a = list(good)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return fn(*a)
        if lib.bpgpu_device_count() == 0:
            assert rc() == m.lib.E_DEVICE, name
        for hole in (0, 1, 2, 3):                                            # context, generators, circuit, program
            assert rc(**{"a%d" % hole: None}) == E, (name, hole)
        for hole in (5, 6, 7, 8, 12, 13, 14, 15):                            # states, label, v, inputs, v_blinding, blindings, points, scalars
            assert rc(**{"a%d" % hole: None}) == E, (name, hole)
        assert rc(a9=None) == E and rc(a10=None) == E                        # one of s_L, s_R
        assert rc(a11=buf) == E and rc(a9=None, a10=None) == E               # both sources, or neither
        assert rc(a20=buf) == E and rc(a20=buf, a21=buf) == E                # some of the witness planes
        for bad in ((4, 1, 2, 1, 1), (3, 2, 3, 1, 1), (3, 1, 2, 0, 1)):      # not the circuit's n, m, nchi
            assert rc(a3=(C.c_size_t * 64)(*bad)) == E, (name, bad)
        assert rc(a2=numeric, a3=(C.c_size_t * 64)(3, 1, 2, 0, 1)) == E, name            # a numeric circuit
        assert rc(a2=two_chi, a3=(C.c_size_t * 64)(3, 1, 2, 2, 1)) == E, name            # nchi != 1
        assert rc(a3=(C.c_size_t * 64)(3, 3, 2, 1, 1)) == m.lib.E_LEN, name              # n1 >= n: no second phase
        assert rc(a1=(C.c_size_t * 64)(2)) == m.lib.E_GENS, name                         # padded n above the capacity
        assert rc(a4=0, a5=None, a6=None, a13=None, a14=None, a15=None) == 0, name       # nb == 0: nothing to do


# ---- bpgpu_witness_plan against the helper's levels
def test_plan_equals_the_helpers_levels_on_every_case():
    import mpc_bulletproof_amd as m
    for case in wc.cases():
        for nb in (1, 65):
            plan = m.lib.witness_plan(*case.prog.plan_args(), nb)
            l1, l2, widest, long_rows = case.prog.levels()
            assert (plan["levels1"], plan["levels2"], plan["widest"], plan["long_rows"], plan["inputs"]) == \
                (l1, l2, widest, long_rows, case.prog.ninp), case.name
            assert (plan["route1"] == 0) == (case.prog.phase1 == 0) and (plan["route2"] == 0) == (case.prog.n == case.prog.phase1), case.name


def test_plan_of_the_gadgets():
    import mpc_bulletproof_amd as m
    for bits, mm in ((8, 1), (64, 3)):
        plan = m.lib.witness_plan(*wc.case("range%dx%d" % (bits, mm)).prog.plan_args(), 4)
        assert (plan["levels1"], plan["levels2"], plan["widest"]) == (1, 0, bits * mm)         # a range program is one level
    assert m.lib.witness_plan(*wc.case("range64x3").prog.plan_args(), 4)["route1"] == 2         # ... wide enough for the block form
    assert m.lib.witness_plan(*wc.case("range64x3").prog.plan_args(), 1 << 16)["route1"] == 2   # 64 rounds of blocks, 192 gates a level
    assert m.lib.witness_plan(*wc.case("range8x1").prog.plan_args(), 1 << 16)["route1"] == 1    # ... against 8
    assert m.lib.witness_plan(*wc.case("gen1").prog.plan_args(), 1)["route1"] == 1              # one gate: a lane
    for k in (2, 3, 4, 9):
        plan = m.lib.witness_plan(*wc.case("shuffle%d" % k).prog.plan_args(), 4)
        assert (plan["levels1"], plan["levels2"], plan["widest"], plan["route2"]) == (0, k - 1, 2, 2), k   # k - 1 levels of width 2
        many = m.lib.witness_plan(*wc.case("shuffle%d" % k).prog.plan_args(), 1025)
        assert many["route2"] == 1 and dict(many, route2=2) == plan        # two rounds of blocks: width 2 no longer pays
    plan = m.lib.witness_plan(*wc.case("composite").prog.plan_args(), 4)
    assert (plan["levels1"], plan["levels2"], plan["inputs"]) == (1, wc.COMPOSITE_K - 1, 2)
    edges = m.lib.witness_plan(*wc.case("edges").prog.plan_args(), 4)
    assert edges["long_rows"] == wc.case("edges").prog.levels()[3] >= 4                           # the 257-term rows are long
    assert m.lib.witness_plan(*wc.case("wide300").prog.plan_args(), 4)["widest"] == 300
    # the route never depends on anything but the shape and nb
    a = m.lib.witness_plan(*wc.case("wide300").prog.plan_args(), 4)
    assert a == m.lib.witness_plan(*wc.case("wide300").prog.plan_args(), 4)
    with pytest.raises(m.BpGpuError):
        m.lib.witness_plan(2, 2, 0, [0, 0], [0, 1, 1, 1, 1], [0], [1], 1)                         # a forward reference


# ---- the cases themselves
def test_evaluator_reproduces_the_model_provers_witness_and_it_satisfies_the_circuit():
    for case in wc.gadget_cases():
        for p in range(len(case.provers)):
            pv = case.model(p)
            assert (pv.a_L, pv.a_R, pv.a_O) == tuple(case.want(p)), (case.name, p)
            assert all(pv.eval(lc) == 0 for lc in pv.constraints), (case.name, p)
            assert all(l * r % N == o for l, r, o in zip(pv.a_L, pv.a_R, pv.a_O))
            assert len(pv.a_L) == case.prog.n


def test_parametric_circuit_of_a_case_serves_every_prover_of_it():
    """circuit_csr (the handle the GPU chain test checks against) is built from prover 0's constraints with the challenge moved to
    the chi block: its rows vanish on every prover's witness and challenge"""
    for case in wc.gadget_cases():
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


def test_broken_inputs_do_not_satisfy_the_circuit():
    for case in wc.gadget_cases():
        v, inputs, chi = case.prover(0)
        v2, inputs2 = case.breaker(v, inputs)
        broken = wc.Case(case.name, case.prog, [(v2, inputs2, chi)], case.gadget)
        pv = broken.model(0)
        assert (pv.a_L, pv.a_R, pv.a_O) == tuple(broken.want(0)), case.name       # still the gadget's witness ...
        assert any(pv.eval(lc) for lc in pv.constraints), case.name               # ... of a statement that does not hold


def test_phases_compose():
    for case in wc.cases():
        v, inputs, chi = case.prover(0)
        first = case.prog.evaluate(v, inputs, chi, phase=1)
        assert tuple(case.prog.evaluate(v, inputs, chi, phase=2, planes=first)) == tuple(case.want(0)), case.name


def test_generated_cases_cover_what_they_claim():
    edges = wc.case("edges").prog
    lengths = {edges.row_len(row) for _, _, left, right in edges.gates for row in (left, right)}
    assert set(wc.ROW_LENGTHS) <= lengths and edges.nchi == 3
    assert {g[1] for g in edges.gates if g[0] == wc.BIT} >= {0, 63, 251}
    aL, aR, _ = wc.case("edges").want(0)
    assert [aR[i] for i in range(0, 6, 2)] == [((N - 1) >> b) & 1 for b in (0, 63, 251)] == [aR[i] for i in (7, 8, 9)]
    assert wc.case("gen1").prog.n == 1 and wc.case("gen70dense").prog.n == 70
    ops = {g[0] for c in wc.generated_cases() for g in c.prog.gates}
    assert ops == {wc.MUL, wc.INPUT, wc.BIT}
    assert wc.case("gen70dense").prog.levels()[0] + wc.case("gen70dense").prog.levels()[1] > 8     # dense back-references: deep
