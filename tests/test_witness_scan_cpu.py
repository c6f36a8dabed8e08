"""The scan pieces of csrc/witness_scan.cuh (wit_scan_local, wit_part_combine, wit_scan_apply: what every thread of k_witness_scan
runs) compiled for the CPU with -fsanitize=undefined as a stand-alone program (tests/csrc/witness_scan_host_test.cpp) that drives them
with T emulated threads in waves of W, and compared with Python integers on every gate: the chain programs of
tests/witness_chain_cases.py, the reference's chain gadgets, and one chain whose every factor is lazily n - 1.  Nothing is loaded
into Python."""
import os
import subprocess

import pytest

import witness_cases as wc
import witness_chain_cases as cc
from test_witness_cpu import text_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THREADS = ((4, 2), (256, 64))          # (T, W): two waves of two lanes, and the kernel's four waves of 64


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    prog = os.path.join(out, "witness_scan_host_test")
    src = os.path.join(HERE, "csrc", "witness_scan_host_test.cpp")
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
    for T, W, prog, v, inputs, chi in jobs:
        lines.append("%x %x" % (T, W))
        lines += text_of(prog, v, inputs, chi)
        lists = cc.scan_lists(prog)
        lines.append("%x" % len(lists))
        for gates, elems in lists:
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


def test_chain_programs(exe, tmp_path):
    """every new program, every prover, both thread counts: byte equality on every gate"""
    check(exe, tmp_path, cc.cases())


def test_reference_gadgets_and_programs_without_a_chain(exe, tmp_path):
    """the shuffles and the composite (short chains), and the programs that have none: the compressed levels are then the levels"""
    check(exe, tmp_path, wc.cases())


def test_chain_of_factors_that_are_lazily_n_minus_one(exe, tmp_path):
    case = cc.lazy_chain_case()
    check(exe, tmp_path, [case])
    import lazy_sum_cases as lz
    assert case.want(0)[2] == [pow(lz.C, i + 1, wc.N) for i in range(case.prog.n)]        # the head and every factor: -2^-261


def test_program_refuses_what_the_library_would(exe, tmp_path):
    """the harness itself: an element whose link row is not one term, and an element out of range, end the program"""
    base = "1\n4 2\n2 1 0 0\n1\n0 0 1 1\n3 0 0 1\n4 0 0 1\n0 0 2 1\n2 0 0 1\n3 0 0 1\n3 0 0 1\n1\n"
    for lists, code in (("1 1\n0\n%x\n" % (1 | cc.ELEM_START), 5), ("1 1\n0\n%x\n" % (2 | cc.ELEM_START), 5), ("2 0\n0\n1\n", 0)):
        path = tmp_path / "bad.txt"
        path.write_text(base + lists)
        assert subprocess.run([exe, str(path)], capture_output=True, timeout=60).returncode == code
