"""bpgpu_witness_chains and the scan route of bpgpu_witness_plan on the CPU: the entry point is exported, bound and declared for
Rust; its figures equal the definition restated in tests/witness_chain_cases.py on every program of the witness tests; the plans of
the programs the library had before are what they were; and the refusals are bpgpu_witness_plan's.  No GPU needed."""
import os
import re

import pytest

import witness_cases as wc
import witness_chain_cases as cc

N = wc.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("chains1", "chains2", "members1", "members2", "longest1", "longest2", "levels1", "levels2")


def _m():
    import mpc_bulletproof_amd as m
    return m


def test_entry_point_option_and_constants_are_exported_bound_and_declared():
    m = _m()
    from mpc_bulletproof_amd._abi import PROTOS
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    name = "bpgpu_witness_chains"
    assert hasattr(m.lib._lib, name) and name in m.lib.SYMBOLS
    decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
    assert decl and len(decl.group(1).split(",")) == 8 and "int32_t out[BPGPU_WIT_CHAIN_FIELDS]" in decl.group(1)
    rdecl = re.search(r"pub fn %s\(([^;]*)\)\s*->" % name, rs, re.S)
    assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == 8
    assert len(PROTOS[name][1]) == 8 and getattr(m.lib._lib, name).argtypes == PROTOS[name][1]
    assert callable(m.BpGpu.witness_chains) and m.lib.WIT_CHAIN_FIELDS == FIELDS
    assert "#define BPGPU_WIT_CHAIN_FIELDS 8" in hdr and "pub const BPGPU_WIT_CHAIN_FIELDS: c_int = 8;" in rs
    for k, f in enumerate(FIELDS):
        assert "#define BPGPU_WIT_CHAIN_%s %d" % (f.upper(), k) in hdr, f
    assert m.lib.OPT["witness_scan_min"] == 21 and "#define BPGPU_OPT_WITNESS_SCAN_MIN 21" in hdr
    assert "#define BPGPU_OPT_COUNT 22" in hdr and "pub const BPGPU_OPT_COUNT: c_int = 22;" in rs
    assert "#define BPGPU_WIT_PLAN_FIELDS 7" in hdr                                  # callers hold 7-int buffers
    text = " ".join(hdr.replace("*", " ").split())
    for phrase in ("product chain", "prefix product", "BPGPU_OPT_WITNESS_SCAN_MIN", "BPGPU_WITNESS_SCAN_MIN", "still serial"):
        assert phrase in text, phrase


def test_chain_figures_equal_the_restated_definition_on_every_program():
    m = _m()
    progs = [c.prog for c in wc.cases()] + [c.prog for c in cc.cases()] + [cc.lazy_chain_case().prog, cc.shuffle(300).prog, cc.shuffle(1 << 14).prog]
    for prog in progs:
        got = m.lib.witness_chains(*prog.plan_args())
        assert got == cc.figures(prog), prog.n
        assert tuple(got) == FIELDS


def test_chain_figures_of_the_gadgets_and_the_new_programs():
    m = _m()

    def fig(prog):
        f = m.lib.witness_chains(*prog.plan_args())
        return (f["chains1"] + f["chains2"], f["members1"] + f["members2"], max(f["longest1"], f["longest2"])), (f["levels1"], f["levels2"])
    for k in (3, 4, 9, 300, 1 << 14):
        prog = wc.case("shuffle%d" % k).prog if k < 10 else cc.shuffle(k).prog
        assert fig(prog) == ((2, 2 * (k - 2), k - 2), (0, 1)), k           # two chains of k - 2 members, ONE compressed level
    assert fig(cc.shuffle(1 << 14).prog) == ((2, 32764, 16382), (0, 1))
    assert fig(wc.case("shuffle2").prog) == ((0, 0, 0), (0, 1))
    assert fig(wc.case("shuffle9").prog)[0][2] == 7 and fig(wc.case("composite").prog)[0] == (2, 2, 1)
    for case in wc.cases():
        if not case.name.startswith(("shuffle", "composite")):
            f = m.lib.witness_chains(*case.prog.plan_args())
            assert (f["chains1"], f["chains2"], f["members1"], f["members2"]) == (0, 0, 0, 0), case.name
            l1, l2 = case.prog.levels()[:2]
            assert (f["levels1"], f["levels2"]) == (l1, l2), case.name     # nothing to compress
    for count in cc.CHAIN_MS:
        assert fig(cc.case("chain%d" % count).prog) == ((1, count, count), (0, 1)), count
    assert fig(cc.case("segments").prog) == ((5, sum(cc.SEGMENTS), max(cc.SEGMENTS)), (1, 0))
    assert fig(cc.case("long2x%d" % cc.LONG).prog) == ((2, 2 * cc.LONG, cc.LONG), (0, 1))
    assert fig(cc.lazy_chain_case().prog) == ((1, 300, 300), (1, 0))


def test_mixed_program_holds_what_it_claims():
    """tests/witness_chain_cases.py mixed_case, read back through the restated definition: which gates are members, on which side,
    and at which compressed level the gates around them sit"""
    case = cc.case("mixed")
    prog, mk = case.prog, case.mark
    pred, right, f = cc.analyse(prog)
    a, b, c, d, e = mk["a"], mk["b"], mk["c"], mk["d"], mk["e"]
    assert [pred[i] for i in a] == [mk["g4"]] + list(a[:-1]) and [right[i] for i in a] == [False, True, False, True, False]
    assert [pred[i] for i in b] == [mk["g_in"], b[0], b[1]] and right[b[1]] and prog.row_len(prog.gates[b[1]][2]) == 257
    assert [pred[i] for i in c] == [mk["g_bit"], c[0], c[1]] and prog.gates[mk["g_bit"]][0] == wc.BIT and prog.gates[mk["g_in"]][0] == wc.INPUT
    assert pred[d[0]] == mk["g2"] and pred[d[1]] is None and pred[d[2]] == d[1]             # two gates linking to one a_O
    assert pred[mk["g3"]] is None and all(pred[i] is None for i in mk["x"])
    assert [pred[i] for i in e] == [mk["h"]] + list(e[:-1]) and pred[mk["y1"]] is None
    assert f == {"chains": (5, 1), "members": (13, 4), "longest": (5, 4), "levels": (4, 2)}
    # the head of chain A sits at level 2, so the gate that reads A's members at level 3; uncompressed the phase is deeper
    assert prog.levels()[0] == 2 + 5 + 1 + 1 and prog.levels()[1] == 6
    for p in range(len(case.provers)):
        aL, aR, aO = case.want(p)
        v, inputs, chi = case.prover(p)
        assert aO[a[1]] != 0 and all(aO[i] == 0 for i in a[2:]) and aR[a[2]] == 0             # a free row that is 0 in mid-chain
        assert all(aO[i] == 0 for i in c[1:]) and aL[c[1]] == 0                               # an explicit zero coefficient
        assert aL[e[0]] == 7 * chi[0] * aO[mk["h"]] % N                                      # a coefficient stored only in a chi block
    assert any(case.want(p)[2][e[3]] for p in range(len(case.provers)))


def test_plans_of_the_earlier_programs_have_not_moved():
    m = _m()
    for case in wc.cases():
        for nb in (1, 4, 65, 1025, 1 << 16):
            plan = m.lib.witness_plan(*case.prog.plan_args(), nb)
            assert plan == cc.parent_plan(case.prog, nb), (case.name, nb)
            assert plan["route1"] in (0, 1, 2) and plan["route2"] in (0, 1, 2), case.name


def test_plan_scans_long_chains_and_depends_on_shape_and_nb_alone():
    m = _m()
    big = cc.shuffle(1 << 14).prog
    plan = m.lib.witness_plan(*big.plan_args(), 1)
    assert plan["route2"] == 3 and plan["route1"] == 0
    assert dict(plan, route2=2) == cc.parent_plan(big, 1)                  # the other six fields are the uncompressed ones
    assert plan == m.lib.witness_plan(*big.plan_args(), 1)
    # the same shape with other coefficients and values: the same plan and the same chains
    one, other = cc.chain_case(257).prog, cc.case("chain257").prog
    other_coeffs = wc.Program(one.m, one.nchi)
    other_coeffs.end_phase1()
    for op, arg, left, right in one.gates:
        other_coeffs.mul([(k, i, tuple(None if p is None else 5 for p in one.parts(c))) for k, i, c in left],
                         [(k, i, tuple(None if p is None else 0 for p in one.parts(c))) for k, i, c in right])
    for nb in (1, 256):
        assert m.lib.witness_plan(*one.plan_args(), nb) == m.lib.witness_plan(*other.plan_args(), nb) == \
            m.lib.witness_plan(*other_coeffs.plan_args(), nb)
    assert m.lib.witness_chains(*one.plan_args()) == m.lib.witness_chains(*other_coeffs.plan_args())
    assert m.lib.witness_plan(*cc.case("long2x%d" % cc.LONG).prog.plan_args(), 1)["route2"] == 3


def test_refusals_are_those_of_the_plan():
    m = _m()
    E = m.lib.E_ARG
    lib = m.lib._lib
    import ctypes as C
    u32 = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs)      # noqa: E731
    out = (C.c_int32 * 8)()
    good = (2, 2, 0, bytes([0, 0]), u32([0, 1, 2, 3, 4]), u32([3, 4, 2, 3]), u32([0, 0, 0, 1]))
    assert lib.bpgpu_witness_chains(*good, out) == 0 and list(out) == [1, 0, 1, 0, 1, 0, 1, 0]
    with pytest.raises(m.BpGpuError) as e:
        m.lib.witness_chains(2, 2, 0, [0, 0], [0, 1, 1, 1, 1], [0], [1])                      # a forward reference
    assert e.value.code == E
    assert lib.bpgpu_witness_chains(2, 2, 0, bytes([0, 0]), None, u32([3]), u32([0]), out) == E         # a null row_ptr
    assert lib.bpgpu_witness_chains(2, 2, 9, bytes([0, 0]), u32([0] * 41), u32([3]), u32([0]), out) == E  # nchi > 8
    assert lib.bpgpu_witness_chains(*good, None) == E
    for bad in ((2, 3, 0), ):                                                                  # n1 > n
        assert lib.bpgpu_witness_chains(*bad, *good[3:], out) == E
    assert lib.bpgpu_witness_chains(1 << 25, 0, 0, bytes(1), u32([0]), None, None, out) == m.lib.E_LEN
