"""The row evaluation of csrc/fn_dev.cuh (eval_row: what every lane of bpgpu_r1cs_constraints_satisfied and
bpgpu_mpc_constraints_eval runs) compiled for the CPU with -fsanitize=undefined as a stand-alone program
(tests/csrc/rows_host_test.cpp) and compared with Python integers: rows around the lazy sums' reduction every 16th term, the heaviest
sums the accumulation can meet (every product lazily n - 1: tests/lazy_sum_cases.py), zero coefficients, a repeated variable and
parametric terms at the edges of the field."""
import os
import random
import subprocess

import pytest

import lazy_sum_cases as lz
import satisfied_cases as sc

N = sc.N
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 257)


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    prog = os.path.join(out, "rows_host_test")
    src = os.path.join(HERE, "csrc", "rows_host_test.cpp")
    hdrs = [os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", f) for f in ("fe29.cuh", "fn_dev.cuh", "kernels.h", "fe29_consts.h")]
    if not os.path.exists(prog) or any(os.path.getmtime(f) > os.path.getmtime(prog) for f in [src] + hdrs):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                               "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", prog, src])
    return prog


def run(exe, tmp_path, cases):
    """cases: (terms [(kind, idx, j, coeff)], values, chi, one) -> [(lane result, wave result)]; and the model's value of each"""
    lines = ["%x" % len(cases)]
    want = []
    for terms, vals, chi, one in cases:
        lines.append("%x %x %x %x" % (len(terms), len(vals), len(chi), one))
        lines += ["%x" % x for x in list(chi) + list(vals)]
        lines += ["%x %x %x %x" % t for t in terms]
        want.append(sum(c * (chi[j - 1] if j else 1) * (one if kind == 4 else vals[idx]) for kind, idx, j, c in terms) % N)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [tuple(int(x, 16) for x in line.split()) for line in r.stdout.split("\n") if line]
    assert len(got) == len(cases)
    return got, want


def test_row_evaluation_equals_the_model(exe, tmp_path):
    rnd = random.Random(2024)
    vals = [0, 1, N - 1] + [rnd.randrange(N) for _ in range(9)]
    cases = []
    for length in LENGTHS:
        # random terms over every kind, the constant included
        cases.append(([(rnd.randrange(5), rnd.randrange(len(vals)), 0, rnd.choice((0, 1, N - 1, rnd.randrange(N)))) for _ in range(length)],
                      vals, (), 1))
        # the heaviest lazy sums: coefficient x value = -2^-261, every product lazily n - 1, through a plane and through chi
        cases.append(([(0, 3, 0, lz.C * lz.inv(vals[3]) % N)] * length, vals, (), 1))
        cases.append(([(k % 4, 3 + k % 9, 0, lz.C * lz.inv(vals[3 + k % 9]) % N) for k in range(length)], vals, (), 1))
        cases.append(([(1, 4, 2, lz.C * lz.inv(vals[4] * vals[5]) % N)] * length, vals, (1, vals[5], 1), 1))
        # every product (n - 1) x (n - 1): lazily 2^261 mod n, a 251-bit value
        cases.append(([(0, 2, 0, N - 1)] * length, vals, (), 1))
        # coefficient 0 throughout; one variable repeated
        cases.append(([(rnd.randrange(4), rnd.randrange(len(vals)), 0, 0) for _ in range(length)], vals, (), 1))
        cases.append(([(1, 5, 0, rnd.randrange(N)) for _ in range(length)], vals, (), 1))
        # parametric terms, chi at the edges: every term scaled by one of chi_1..chi_3 or by none
        for chi in ((0, 0, 0), (1, 1, 1), (N - 1, N - 1, N - 1), (0, 1, N - 1)):
            cases.append(([(rnd.randrange(5), rnd.randrange(len(vals)), rnd.randrange(4), rnd.choice((1, N - 1, rnd.randrange(N))))
                           for _ in range(length)], vals, chi, 1))
        cases.append(([(0, 2, 3, N - 1)] * length, vals, (N - 1, N - 1, N - 1), 1))
        # a share or MAC plane of the two-party evaluation: the constant reads 0
        cases.append(([(4, 0, 0, rnd.randrange(1, N))] * length + [(2, 7, 0, 3)], vals, (), 0))
    got, want = run(exe, tmp_path, cases)
    for i, ((lane, wave), w) in enumerate(zip(got, want)):
        assert lane == w and wave == w, (i, len(cases[i][0]))


def test_program_refuses_a_non_canonical_value(exe, tmp_path):
    """the harness itself: a value of n is not canonical and the program says so instead of evaluating it"""
    path = tmp_path / "bad.txt"
    path.write_text("1\n1 1 0 1\n%x\n0 0 0 1\n" % N)
    assert subprocess.run([exe, str(path)], capture_output=True, timeout=60).returncode == 4
