"""The integer division of csrc/int_div.cuh and the DIVREM gate of csrc/witness_dev.cuh (wit_gate_values_of / wit_gate_store_of: what
every lane of csrc/k_witness.hip runs) compiled for the CPU with -fsanitize=undefined as a stand-alone program
(tests/csrc/witness_divrem_host_test.cpp) and compared with Python integers: every program of tests/witness_divrem_cases.py gate by
gate, and the bare division on seeded random pairs of random bit lengths and on the crafted pairs of the case file.  Nothing is
loaded into Python."""
import os
import random
import subprocess

import pytest

import witness_cases as wc
import witness_divrem_cases as dc
from test_witness_cpu import text_of

N = wc.N
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RANDOM_PAIRS = 100000


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    prog = os.path.join(out, "witness_divrem_host_test")
    src = os.path.join(HERE, "csrc", "witness_divrem_host_test.cpp")
    hdrs = [os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", f)
            for f in ("fe29.cuh", "fn_dev.cuh", "int_div.cuh", "witness_dev.cuh", "kernels.h", "fe29_consts.h")]
    if not os.path.exists(prog) or any(os.path.getmtime(f) > os.path.getmtime(prog) for f in [src] + hdrs):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                               "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", prog, src])
    return prog


def run_programs(exe, tmp_path, jobs):
    """jobs: (program, v, inputs, chi) -> per job, per gate, the six values the program printed"""
    lines = ["%x" % len(jobs)]
    for job in jobs:
        lines += text_of(*job)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "prog", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [tuple(int(x, 16) for x in line.split()) for line in r.stdout.split("\n") if line]
    assert len(got) == sum(job[0].n for job in jobs)
    out, at = [], 0
    for job in jobs:
        out.append(got[at:at + job[0].n])
        at += job[0].n
    return out


def run_division(exe, tmp_path, pairs):
    path = tmp_path / "pairs.txt"
    path.write_text("%x\n" % len(pairs) + "".join("%x %x\n" % p for p in pairs))
    r = subprocess.run([exe, "div", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [tuple(int(x, 16) for x in line.split()) for line in r.stdout.split("\n") if line]
    assert len(got) == len(pairs)
    return got


def check_division(pairs, got):
    for (x, y), (q, r) in zip(pairs, got):
        assert (q, r) == dc.divrem(x, y), (hex(x), hex(y))
        assert x == q * y + r and (y == 0 or r < y), (hex(x), hex(y))


def test_the_cases_contain_what_they_claim():
    dc.self_check()


def test_every_program_of_the_case_file_gate_by_gate(exe, tmp_path):
    """every prover of every case, in the gate-by-gate form and with the long rows summed from 64 lane parts"""
    jobs = [(case.prog,) + pr for case in dc.cases() for pr in case.provers]
    got = run_programs(exe, tmp_path, jobs)
    at = 0
    for case in dc.cases():
        for p in range(len(case.provers)):
            aL, aR, aO = case.want(p)
            for i, row in enumerate(got[at]):
                assert row == (aL[i], aR[i], aO[i]) * 2, (case.name, p, i, case.prog.gates[i][:2])
            at += 1


def test_bare_division_on_random_pairs_of_random_bit_lengths(exe, tmp_path):
    """RANDOM_PAIRS seeded pairs, each operand of a bit length drawn from 0 .. 256 (the routine takes any 8 words): against divmod,
    and against the identity with the remainder's bound"""
    rnd = random.Random(20261021)
    pairs = []
    for _ in range(RANDOM_PAIRS):
        bx, by = rnd.randrange(257), rnd.randrange(257)
        pairs.append((rnd.getrandbits(bx) if bx else 0, rnd.getrandbits(by) if by else 0))
    assert len(pairs) >= 10 ** 5 and any(y == 0 for _, y in pairs) and any(x < y for x, y in pairs)
    check_division(pairs, run_division(exe, tmp_path, pairs))


def test_bare_division_on_the_crafted_pairs(exe, tmp_path):
    """the edges, the bit lengths (both kinds of value, and mixed) and the schoolbook digits of the case file, and the largest words"""
    values = list(dc.EDGES) + dc.bitlen_values(True) + dc.bitlen_values(False) + [(1 << 256) - 1, 1 << 255, (1 << 256) - (1 << 32)]
    pairs = [(x, y) for x in values for y in values] + dc.digit_pairs()
    check_division(pairs, run_division(exe, tmp_path, pairs))


def test_program_refuses_what_the_library_would(exe, tmp_path):
    """the harness itself: ops 3, 5 and 7 end the program instead of being evaluated"""
    for op in (3, 5, 7):
        path = tmp_path / "bad.txt"
        path.write_text("1\n1 1 0 0\n1\n%x 0 1 0\n3 0 0 1\n" % op)
        assert subprocess.run([exe, "prog", str(path)], capture_output=True, timeout=60).returncode == 5
    path = tmp_path / "good.txt"
    path.write_text("1\n1 1 0 0\n7\n6 0 1 1\n3 0 0 1\n4 0 0 2\n")
    r = subprocess.run([exe, "prog", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and [int(x, 16) for x in r.stdout.split()] == [3, 1, 3] * 2
