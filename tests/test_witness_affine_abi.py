"""bpgpu_witness_affine_chains and the widened scan route of bpgpu_witness_plan on the CPU: the entry point is exported, bound and
declared for Rust; its figures equal the definition restated in tests/witness_affine_cases.py on every program of the witness tests;
bpgpu_witness_chains is unmoved on the new programs; a long Horner gadget is planned into the scan form and a short one is not; and
the refusals are bpgpu_witness_plan's.  No GPU needed."""
import os
import re

import pytest

import witness_cases as wc
import witness_chain_cases as cc
import witness_affine_cases as ac

N = wc.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _m():
    import mpc_bulletproof_amd as m
    return m


def test_entry_point_and_constants_are_exported_bound_and_declared():
    m = _m()
    from mpc_bulletproof_amd._abi import PROTOS
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    name = "bpgpu_witness_affine_chains"
    assert hasattr(m.lib._lib, name) and name in m.lib.SYMBOLS
    decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
    assert decl and len(decl.group(1).split(",")) == 8 and "int32_t out[BPGPU_WIT_AFF_FIELDS]" in decl.group(1)
    rdecl = re.search(r"pub fn %s\(([^;]*)\)\s*->" % name, rs, re.S)
    assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == 8
    assert len(PROTOS[name][1]) == 8 and getattr(m.lib._lib, name).argtypes == PROTOS[name][1]
    assert callable(m.BpGpu.witness_affine_chains) and m.lib.WIT_AFF_FIELDS == ac.FIELDS
    assert "#define BPGPU_WIT_AFF_FIELDS 10" in hdr and "pub const BPGPU_WIT_AFF_FIELDS: c_int = 10;" in rs
    for k, f in enumerate(ac.FIELDS):
        assert "#define BPGPU_WIT_AFF_%s %d" % (f.upper(), k) in hdr, f
    # no new option, no new plan field, and the product diagnostic as it was
    assert "#define BPGPU_OPT_COUNT 22" in hdr and "#define BPGPU_WIT_PLAN_FIELDS 7" in hdr and "#define BPGPU_WIT_CHAIN_FIELDS 8" in hdr
    text = " ".join(hdr.replace("*", " ").split())
    for phrase in ("affine member", "prefix composition", "bpgpu_witness_affine_chains", "still serial", "split over"):
        assert phrase in text, phrase


def test_figures_equal_the_restated_definition_on_every_program():
    m = _m()
    progs = [c.prog for c in wc.cases() + cc.cases() + ac.cases()] + [cc.lazy_chain_case().prog, cc.shuffle(300).prog, ac.horner_case(40).prog]
    for prog in progs:
        got = m.lib.witness_affine_chains(*prog.plan_args())
        assert got == ac.figures(prog), prog.n
        assert tuple(got) == ac.FIELDS
        # the product diagnostic is pass 1's, whatever pass 2 adds
        assert m.lib.witness_chains(*prog.plan_args()) == cc.figures(prog), prog.n


def test_a_program_without_an_affine_member_reports_its_product_chains():
    m = _m()
    for case in wc.cases() + cc.cases():
        ext, prod = m.lib.witness_affine_chains(*case.prog.plan_args()), m.lib.witness_chains(*case.prog.plan_args())
        if case.name == "gen70dense":                                         # two affine members, in chains of length 1
            assert (ext["affine1"], ext["affine2"], ext["longest1"], ext["longest2"]) == (1, 1, 1, 1)
            continue
        assert ext["affine1"] == ext["affine2"] == 0, case.name
        assert {k: v for k, v in ext.items() if not k.startswith("affine")} == prod, case.name


def test_figures_of_the_new_programs():
    m = _m()

    def fig(prog):
        f = m.lib.witness_affine_chains(*prog.plan_args())
        return tuple(f[k + "1"] + f[k + "2"] for k in ("chains", "members", "affine")), max(f["longest1"], f["longest2"]), (f["levels1"], f["levels2"])
    for k in (2, 3, 9, 40, 300):
        prog = ac.horner_case(k).prog
        assert prog.n == 2 * (k - 1) and prog.levels()[:2] == (0, k - 1)
        chains = 2 if k > 2 else 0
        assert fig(prog) == ((chains, 2 * (k - 2), 2 * (k - 2)), k - 2, (0, 1)), k           # two chains of k - 2 members, ONE level
    for count in ac.CHAIN_MS:
        assert fig(ac.case("affine%d" % count).prog) == ((1, count, count), count, (0, 1)), count
    assert fig(ac.case("affsegments").prog) == ((5, sum(ac.SEGMENTS), 3 + 2), max(ac.SEGMENTS), (1, 0))
    assert fig(ac.case("afflong2x%d" % ac.LONG).prog) == ((2, 2 * ac.LONG, 2 * ac.LONG), ac.LONG, (0, 1))
    assert fig(ac.case("afflazy300").prog) == ((1, 300, 300), 300, (1, 0))
    assert m.lib.witness_affine_chains(*ac.case("affmixed").prog.plan_args()) == dict(
        chains1=5, chains2=1, members1=13, members2=3, affine1=8, affine2=3, longest1=7, longest2=3, levels1=3, levels2=3)


def test_mixed_program_holds_what_it_claims():
    """tests/witness_affine_cases.py mixed_case, read back through the restated definition: which gates are members, of which kind, on
    which side, and what the values around a zero are"""
    case = ac.case("affmixed")
    prog, mk = case.prog, case.mark
    pred, right, affine, level, _ = ac.analyse(prog)
    prod = cc.analyse(prog)[0]
    a, p, q, d, e = mk["a"], mk["p"], mk["q"], mk["d"], mk["e"]
    h1, h2 = mk["h12"]
    assert [pred[i] for i in a] == [mk["g1"]] + list(a[:-1])                                 # one chain mixing the kinds
    assert [affine[i] for i in a] == [False, True, True, True, False, True, True]
    assert [right[i] for i in a] == [False, True, False, False, True, False, True]
    # a product gate and an affine gate competing for one a_O: the product gate is the member, whatever the order
    assert pred[p[0]] is None and pred[p[1]] == mk["g0"] and not affine[p[1]] and prod[p[1]] == mk["g0"]
    assert pred[q[1]] == q[0] and not affine[q[1]] and pred[q[2]] is None
    # two gates affine-linking to one a_O: the first is the member; the second heads d3, h1 and h2
    assert pred[d[1]] == d[0] and affine[d[1]] and pred[d[2]] is None and pred[d[3]] == d[2] and affine[d[3]] and right[d[3]]
    assert prod[h1] is None and prod[h2] == h1                                               # pass 1: h1 a head ...
    assert pred[h1] == d[3] and affine[h1] and pred[h2] == h1 and not affine[h2]             # ... pass 2: a member
    assert level[d[2]] == level[d[3]] == level[h1] == level[h2] == 1
    assert all(pred[i] is None for i in mk["s"] + (mk["x1"], mk["y1"], mk["h"]))
    assert [pred[i] for i in e[:3]] == [mk["h"], e[0], e[1]] and all(affine[i] for i in e[:3]) and [right[i] for i in e[:3]] == [False, True, False]
    assert pred[e[3]] is None and len(cc._stored(prog, prog.gates[e[3]][2])) == 3             # a link coefficient split over two blocks
    for pr in range(len(case.provers)):
        aL, aR, aO = case.want(pr)
        v, _, chi = case.prover(pr)
        assert aR[a[2]] == 0 and aO[a[2]] == 0 and aO[a[1]] != 0                             # g = 0 in mid-chain ...
        assert aO[a[3]] == (7 + v[2]) * aR[a[3]] % N != 0                                    # ... the next member is B alone
        assert aL[a[5]] == v[1] and aO[a[5]] == v[1] * aR[a[5]] % N                          # an explicit zero link coefficient
        assert aL[e[0]] == (7 * chi[0] * aO[mk["h"]] + aO[a[6]]) % N                         # a coefficient stored only in a chi block
    assert any(case.want(pr)[2][e[2]] for pr in range(len(case.provers)))


def test_plan_scans_a_long_horner_gadget_and_leaves_a_short_one():
    m = _m()
    big = ac.horner_case(300).prog
    assert m.lib.witness_chains(*big.plan_args())["longest2"] == 0          # no product chain: the parent planned 1 or 2
    for nb in (1, 256):
        plan = m.lib.witness_plan(*big.plan_args(), nb)
        assert plan["route2"] == 3 and plan["route1"] == 0, nb
        assert dict(plan, route2=cc.parent_plan(big, nb)["route2"]) == cc.parent_plan(big, nb)   # the other six fields
    small = ac.horner_case(9).prog
    for nb in (1, 256):
        assert m.lib.witness_plan(*small.plan_args(), nb) == cc.parent_plan(small, nb), nb
    # the plan depends on shape alone: the same shape with other coefficients gives the same plan and the same chains
    other = wc.Program(big.m, big.nchi)
    other.end_phase1()
    for op, arg, left, right in big.gates:
        other.mul([(k, i, tuple(None if p is None else 5 for p in big.parts(c))) for k, i, c in left],
                  [(k, i, tuple(None if p is None else 0 for p in big.parts(c))) for k, i, c in right])
    for nb in (1, 256):
        assert m.lib.witness_plan(*big.plan_args(), nb) == m.lib.witness_plan(*other.plan_args(), nb)
    assert m.lib.witness_affine_chains(*big.plan_args()) == m.lib.witness_affine_chains(*other.plan_args())


def test_refusals_are_those_of_the_plan():
    m = _m()
    E = m.lib.E_ARG
    lib = m.lib._lib
    import ctypes as C
    u32 = lambda xs: (C.c_uint32 * max(len(xs), 1))(*xs)      # noqa: E731
    out = (C.c_int32 * 10)()
    # gate 1: left a_O[0] + v_0 (an affine link), right v_0
    good = (2, 2, 0, bytes([0, 0]), u32([0, 1, 2, 4, 5]), u32([3, 4, 2, 3, 3]), u32([0, 0, 0, 0, 0]))
    assert lib.bpgpu_witness_affine_chains(*good, out) == 0 and list(out) == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    with pytest.raises(m.BpGpuError) as e:
        m.lib.witness_affine_chains(2, 2, 0, [0, 0], [0, 1, 1, 1, 1], [0], [1])                      # a forward reference
    assert e.value.code == E
    assert lib.bpgpu_witness_affine_chains(2, 2, 0, bytes([0, 0]), None, u32([3]), u32([0]), out) == E         # a null row_ptr
    assert lib.bpgpu_witness_affine_chains(2, 2, 9, bytes([0, 0]), u32([0] * 41), u32([3]), u32([0]), out) == E  # nchi > 8
    assert lib.bpgpu_witness_affine_chains(*good, None) == E
    assert lib.bpgpu_witness_affine_chains(2, 3, 0, *good[3:], out) == E                              # n1 > n
    assert lib.bpgpu_witness_affine_chains(1 << 25, 0, 0, bytes(1), u32([0]), None, None, out) == m.lib.E_LEN
