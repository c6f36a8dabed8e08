"""The gate body of csrc/witness_dev.cuh (wit_gate_lane / wit_gate_values: what every lane of bpgpu_r1cs_witness_synthesize runs)
compiled for the CPU with -fsanitize=undefined as a stand-alone program (tests/csrc/witness_host_test.cpp) and compared with Python
integers: the three ops, the heaviest lazy sums (every product lazily n - 1: tests/lazy_sum_cases.py) feeding the gate's product,
rows on the fold boundaries in both launch forms, and the bit extraction at the edges of the field.  Nothing is loaded into Python."""
import os
import random
import subprocess

import pytest

import lazy_sum_cases as lz
import witness_cases as wc

N = wc.N
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 257)
V, ONE, O = wc.V, wc.ONE, wc.O


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    prog = os.path.join(out, "witness_host_test")
    src = os.path.join(HERE, "csrc", "witness_host_test.cpp")
    hdrs = [os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", f) for f in ("fe29.cuh", "fn_dev.cuh", "witness_dev.cuh", "kernels.h", "fe29_consts.h")]
    if not os.path.exists(prog) or any(os.path.getmtime(f) > os.path.getmtime(prog) for f in [src] + hdrs):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                               "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", prog, src])
    return prog


def text_of(prog, v, inputs, chi):
    lines = ["%x %x %x %x" % (prog.n, prog.m, prog.ninp, prog.nchi)]
    lines += ["%x" % x for x in list(chi) + list(v) + [x for pair in inputs for x in pair]]
    pair = 0
    for op, arg, left, right in prog.gates:
        rows = [[(kind, idx, j, part) for kind, idx, coeff in row for j, part in enumerate(prog.parts(coeff)) if part is not None]
                for row in (left, right)]
        lines.append("%x %x %x %x" % (op, pair if op == wc.INPUT else arg, len(rows[0]), len(rows[1])))
        pair += op == wc.INPUT
        lines += ["%x %x %x %x" % t for row in rows for t in row]
    return lines


def run(exe, tmp_path, jobs):
    """jobs: (program, v, inputs, chi) -> per job, per gate, the six values the program printed"""
    lines = ["%x" % len(jobs)]
    for job in jobs:
        lines += text_of(*job)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [tuple(int(x, 16) for x in line.split()) for line in r.stdout.split("\n") if line]
    assert len(got) == sum(job[0].n for job in jobs)
    out, at = [], 0
    for job in jobs:
        out.append(got[at:at + job[0].n])
        at += job[0].n
    return out


def check(got, jobs):
    for g, (prog, v, inputs, chi) in zip(got, jobs):
        aL, aR, aO = prog.evaluate(v, inputs, chi)
        for i, row in enumerate(g):
            assert row == (aL[i], aR[i], aO[i]) * 2, (i, prog.gates[i][:2])


def test_every_case_of_the_gpu_tests(exe, tmp_path):
    """the programs tests/test_gpu_witness.py runs on the device: all three ops, both phases, every prover of every case"""
    jobs = [(case.prog,) + pr for case in wc.cases() for pr in case.provers]
    check(run(exe, tmp_path, jobs), jobs)


def test_heaviest_lazy_sums_feed_the_gate_product(exe, tmp_path):
    """both rows of a gate are sums of `length` products that are each lazily n - 1 (coefficient x value = -2^-261), straight and
    through chi; the gate reduces both before it multiplies, and the next gate reads the product"""
    rnd = random.Random(2025)
    vals = [rnd.randrange(1, N) for _ in range(6)]
    chi = (vals[5], 1, N - 1)
    jobs = []
    for length in LENGTHS:
        prog = wc.Program(len(vals), nchi=3)
        worst = [(V, 3, lz.C * lz.inv(vals[3]) % N)] * length
        mixed = [(V, k % 5, lz.C * lz.inv(vals[k % 5]) % N) for k in range(length)]
        prog.end_phase1()
        prog.mul(worst, mixed)
        prog.mul([(V, 4, (None, lz.C * lz.inv(vals[4] * vals[5]) % N, None, None))] * length, [(V, 2, (None, None, None, lz.C * lz.inv(-vals[2]) % N))] * length)
        prog.mul([(O, 0, N - 1)] * length, [(O, 1, N - 1), (O, 0, 1)] * (length // 2))
        prog.mul([(V, 0, N - 1)] * length + [(ONE, 0, N - 1)], [(ONE, 0, N - 1)] * length)
        prog.bit(worst, 251)
        prog.bit(mixed + [(ONE, 0, 1)], 0)
        jobs.append((prog, vals, (), chi))
    check(run(exe, tmp_path, jobs), jobs)


def test_bit_extraction_at_the_edges_of_the_field(exe, tmp_path):
    """every bit 0..251 of n - 1, of 2^251, of 1 and of 0, read from a value; bits of a sum that wraps past n"""
    values = [N - 1, 1 << 251, 1, 0, (N + 1) // 2]
    prog = wc.Program(len(values))
    for j in range(len(values)):
        for b in range(252):
            prog.bit([(V, j, 1)], b)
    for b in (0, 1, 63, 64, 250, 251):
        prog.bit([(V, 0, 1), (ONE, 0, 2)], b)            # n - 1 + 2 = 1 (mod n)
        prog.bit([(V, 4, 2)], b)                         # 2 (n + 1) / 2 = 1 (mod n)
        prog.bit([(V, 1, 1), (V, 1, 1)], b)              # 2^252 - n
    prog.end_phase1()
    job = (prog, values, (), ())
    got = run(exe, tmp_path, [job])
    check(got, [job])
    assert [row[1] for row in got[0][:252]] == [((N - 1) >> b) & 1 for b in range(252)]


def test_inputs_and_references(exe, tmp_path):
    """INPUT pairs are consumed in gate order, at the edges of the field; a_L, a_R and a_O of earlier gates are read back"""
    prog = wc.Program(1)
    a = prog.input()
    b = prog.input()
    c = prog.mul([(wc.L, a, 1), (wc.R, b, N - 1)], [(wc.O, a, 1), (wc.O, b, 1), (V, 0, 1)])
    prog.input()
    prog.mul([(wc.L, c, 1), (wc.L, 3, 1)], [(wc.R, 3, 1)])
    prog.end_phase1()
    jobs = [(prog, [v0], [(N - 1, N - 1), (x, (N + 1) // 2), (1 << 251, x)], ()) for v0 in (0, N - 1) for x in (0, 1, N - 1)]
    check(run(exe, tmp_path, jobs), jobs)


def test_program_refuses_what_the_library_would(exe, tmp_path):
    """the harness itself: a non-canonical value, a forward reference and a bit of 252 end the program instead of being evaluated"""
    for text, code in (("1\n1 1 0 0\n%x\n0 0 1 0\n3 0 0 1\n" % N, 4), ("1\n1 1 0 0\n1\n0 0 1 0\n0 0 0 1\n", 5), ("1\n1 1 0 0\n1\n2 fc 1 0\n3 0 0 1\n", 5)):
        path = tmp_path / "bad.txt"
        path.write_text(text)
        assert subprocess.run([exe, str(path)], capture_output=True, timeout=60).returncode == code
