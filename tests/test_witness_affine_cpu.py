"""The affine pieces of csrc/witness_scan.cuh (wit_aff_local, wit_aff_combine, wit_aff_apply: what every thread of
k_witness_scan<true> runs) compiled for the CPU with -fsanitize=undefined as a stand-alone program
(tests/csrc/witness_affine_host_test.cpp) that drives them with T emulated threads in waves of W, and compared with Python integers on
every gate of every prover of the programs of tests/witness_affine_cases.py -- the chain in which every A and every B is lazily n - 1
among them -- and of the earlier chain programs, which the affine operator must evaluate as well (a product member is the map with
f = 0).  The extended lists come from the restated definition.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

import witness_cases as wc
import witness_chain_cases as cc
import witness_affine_cases as ac
from test_witness_cpu import text_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THREADS = ((4, 2), (256, 64))          # (T, W): two waves of two lanes, and the kernel's four waves of 64


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    prog = os.path.join(out, "witness_affine_host_test")
    src = os.path.join(HERE, "csrc", "witness_affine_host_test.cpp")
    hdrs = [os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", f)
            for f in ("fe29.cuh", "fn_dev.cuh", "witness_dev.cuh", "witness_scan.cuh", "kernels.h", "fe29_consts.h")]
    if not os.path.exists(prog) or any(os.path.getmtime(f) > os.path.getmtime(prog) for f in [src] + hdrs):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                               "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", prog, src])
    return prog


def run(exe, tmp_path, jobs):
    """jobs: (T, W, program, v, inputs, chi) -> per job, per gate, (a_L, a_R, a_O) as the program printed them"""
    lines = ["%x" % len(jobs)]
    copies, lists = {}, {}
    for T, W, prog, v, inputs, chi in jobs:
        if id(prog) not in copies:
            copies[id(prog)], lists[id(prog)] = ac.library_copy(prog), ac.scan_lists(prog)
        lines.append("%x %x" % (T, W))
        lines += text_of(copies[id(prog)], v, inputs, chi)
        lines.append("%x" % len(lists[id(prog)]))
        for gates, elems in lists[id(prog)]:
            lines.append("%x %x" % (len(gates), len(elems)))
            lines += ["%x" % x for x in gates + elems]
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [tuple(int(x, 16) for x in line.split()) for line in r.stdout.split("\n") if line]
    assert len(got) == sum(job[2].n for job in jobs)
    out, at = [], 0
    for job in jobs:
        out.append(got[at:at + job[2].n])
        at += job[2].n
    return out


def check(exe, tmp_path, cases):
    jobs, want = [], []
    for case in cases:
        for p, pr in enumerate(case.provers):
            for T, W in THREADS:
                jobs.append((T, W, case.prog) + tuple(pr))
                want.append((case.name, p, T, case.want(p)))
    for g, (name, p, T, (aL, aR, aO)) in zip(run(exe, tmp_path, jobs), want):
        for i, row in enumerate(g):
            assert row == (aL[i], aR[i], aO[i]), (name, p, T, i)


def test_affine_programs(exe, tmp_path):
    """every new program, every prover, both thread counts: byte equality on every gate"""
    check(exe, tmp_path, ac.cases())


def test_product_chains_under_the_affine_operator(exe, tmp_path):
    """the earlier chain programs and the reference's gadgets: their members are maps with f = 0 (gen70dense has two affine members)"""
    check(exe, tmp_path, [c for c in cc.cases() if c.name != "long2x%d" % cc.LONG] + wc.cases())


def test_chain_of_maps_that_are_lazily_n_minus_one(exe, tmp_path):
    """every A = c g and every B = f g has the Montgomery residue n - 1, for 300 members: the sums A2 B1 + B2 that feed the next product
    are the heaviest the operator can be handed (the bound above wit_aff_combine)"""
    import lazy_sum_cases as lz
    case = ac.lazy_case()
    assert ac.figures(case.prog)["affine1"] == 300
    check(exe, tmp_path, [case])
    aO, c = case.want(0)[2], lz.C
    assert aO[0] == c and all(aO[i + 1] == (aO[i] + 1) * c % wc.N for i in range(300))          # x -> C x + C from the head's C


def test_program_refuses_what_the_library_would(exe, tmp_path):
    """the harness itself: a product element whose link row is not one term, an affine element whose first term is no a_O term, an
    element out of range and a flag above the three end the program"""
    base = "1\n4 2\n2 1 0 0\n1\n0 0 1 1\n3 0 0 1\n4 0 0 1\n0 0 2 1\n3 0 0 1\n2 0 0 1\n3 0 0 1\n1\n"      # gate 1: left v + a_O[0], right v
    for lists, code in (("1 1\n0\n%x\n" % (1 | ac.ELEM_START), 5), ("1 1\n0\n%x\n" % (1 | ac.ELEM_START | ac.ELEM_AFFINE), 5),
                        ("1 1\n0\n%x\n" % (2 | ac.ELEM_START), 5), ("1 1\n0\n%x\n" % (1 | ac.ELEM_START | 1 << 28), 5), ("2 0\n0\n1\n", 0)):
        path = tmp_path / "bad.txt"
        path.write_text(base + lists)
        assert subprocess.run([exe, str(path)], capture_output=True, timeout=60).returncode == code
