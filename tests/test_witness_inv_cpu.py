"""The INV gate of csrc/witness_dev.cuh (wit_gate_values_of, and the forward / backward passes of the batched inversion that the
block and scan forms of csrc/k_witness.hip run) compiled for the CPU with -fsanitize=undefined as a stand-alone program
(tests/csrc/witness_inv_host_test.cpp) and compared with Python integers: gate by gate, and level by level with 4 and with 256
emulated threads -- the values at the edges of the field, rows that are the heaviest lazy sums of tests/lazy_sum_cases.py, levels of
1 .. 513 INV gates with a zero at every place of a thread's run, and levels of zeros only.  Nothing is loaded into Python."""
import os
import random
import subprocess

import pytest

import lazy_sum_cases as lz
import witness_cases as wc
import witness_inv_cases as ic
from test_witness_cpu import text_of

N = wc.N
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THREADS = (4, 256)
LENGTHS = (1, 15, 16, 17, 33, 64, 257)
V, ONE, O, R = wc.V, wc.ONE, wc.O, wc.R


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    prog = os.path.join(out, "witness_inv_host_test")
    src = os.path.join(HERE, "csrc", "witness_inv_host_test.cpp")
    hdrs = [os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", f) for f in ("fe29.cuh", "fn_dev.cuh", "witness_dev.cuh", "kernels.h", "fe29_consts.h")]
    if not os.path.exists(prog) or any(os.path.getmtime(f) > os.path.getmtime(prog) for f in [src] + hdrs):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                               "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", prog, src])
    return prog


def run(exe, tmp_path, jobs, threads):
    """jobs: (program, v, inputs, chi) -> per job, per gate, the six values the program printed"""
    lines = ["%x" % len(jobs)]
    for job in jobs:
        lines += text_of(*job)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path), str(threads)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [tuple(int(x, 16) for x in line.split()) for line in r.stdout.split("\n") if line]
    assert len(got) == sum(job[0].n for job in jobs)
    out, at = [], 0
    for job in jobs:
        out.append(got[at:at + job[0].n])
        at += job[0].n
    return out


_want = {}


def check(got, jobs, threads):
    for k, (g, (prog, v, inputs, chi)) in enumerate(zip(got, jobs)):
        key = (id(prog), tuple(v), tuple(chi))
        if key not in _want:
            _want[key] = prog.evaluate(v, inputs, chi)          # once, shared by both thread counts
        aL, aR, aO = _want[key]
        for i, row in enumerate(g):
            assert row == (aL[i], aR[i], aO[i]) * 2, (threads, k, i, prog.gates[i][:2])


@pytest.mark.parametrize("threads", THREADS)
def test_every_case_of_the_gpu_tests(exe, tmp_path, threads):
    """the programs tests/test_gpu_witness_inv.py runs on the device, every prover of every case: the edge values, the levels of 1, 3,
    255, 256, 257 and 513 INV gates with their zeros, the long rows, the chain, the challenge"""
    jobs = [(case.prog,) + pr for case in ic.cases() for pr in case.provers]
    check(run(exe, tmp_path, jobs, threads), jobs, threads)


_heavy = []


def heavy_jobs():
    """an INV gate over `length` products that are each lazily n - 1 (coefficient x value = -2^-261), straight and through chi, a level
    of them so that the batched products meet them too, and a second level that reads the inverses"""
    if _heavy:
        return _heavy
    rnd = random.Random(2026)
    vals = [rnd.randrange(1, N) for _ in range(6)]
    chi = (vals[5], 1, N - 1)
    for length in LENGTHS:
        prog = ic.Program(len(vals), nchi=3)
        worst = [(V, 3, lz.C * lz.inv(vals[3]) % N)] * length
        mixed = [(V, k % 5, lz.C * lz.inv(vals[k % 5]) % N) for k in range(length)]
        prog.end_phase1()
        first = prog.n
        for _ in range(5):
            prog.inv(worst)
            prog.inv(mixed)
            prog.inv([(V, 4, (None, lz.C * lz.inv(vals[4] * vals[5]) % N, None, None))] * length)
            prog.inv([(V, 2, (None, None, None, lz.C * lz.inv(-vals[2]) % N))] * length)
            prog.inv(worst + [(ONE, 0, -length * lz.C % N)])          # the heaviest sum that is zero
        for i in range(first, prog.n, 3):
            prog.inv([(R, i, N - 1)] * min(length, 33) + [(O, i, 1)])
        _heavy.append((prog, vals, (), chi))
    return _heavy


@pytest.mark.parametrize("threads", THREADS)
def test_heaviest_lazy_sums_feed_the_inversion(exe, tmp_path, threads):
    jobs = heavy_jobs()
    check(run(exe, tmp_path, jobs, threads), jobs, threads)
    # the case is what it claims: every product of a `worst` row is n - 1 lazily, i.e. -2^-261 mod n as a value
    prog, vals, _, chi = jobs[0]
    assert prog.gates[0][2][0][2] * vals[3] % N == lz.C


def test_inverses_are_inverses(exe, tmp_path):
    """the printed values themselves, apart from the Python model: a_L a_R = a_O in {0, 1}, and a_O = 0 exactly where a_L = 0"""
    case = ic.case("inv_level513")
    jobs = [(case.prog,) + pr for pr in case.provers]
    for g in run(exe, tmp_path, jobs, 256):
        for i, row in enumerate(g[:513]):
            for aL, aR, aO in (row[:3], row[3:]):
                assert aL * aR % N == aO == int(aL != 0) and (aL != 0 or aR == 0), i


def test_program_refuses_what_the_library_would(exe, tmp_path):
    """the harness itself: op 3, op 5 and an INV gate with a right row end the program instead of being evaluated"""
    for text in ("1\n1 1 0 0\n1\n3 0 1 0\n3 0 0 1\n", "1\n1 1 0 0\n1\n5 0 1 0\n3 0 0 1\n", "1\n1 1 0 0\n1\n4 0 1 1\n3 0 0 1\n4 0 0 1\n"):
        path = tmp_path / "bad.txt"
        path.write_text(text)
        assert subprocess.run([exe, str(path), "4"], capture_output=True, timeout=60).returncode == 5
