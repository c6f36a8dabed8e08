"""The gate and plane arithmetic of csrc/mpc_witness_dev.cuh (what every lane of bpgpu_mpc_witness_mask / _combine runs) compiled for
the CPU with -fsanitize=undefined as a stand-alone program (tests/csrc/mpc_witness_host_test.cpp) and compared with the model of
tests/mpc_witness_cases.py on Python integers: every plane of both parties, level by level, in the lane form and the wave form -- rows
on the lazy sums' fold boundaries, a row above a lane's 64 terms, INPUT gates, nchi = 3.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

import mpc_witness_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    prog = os.path.join(out, "mpc_witness_host_test")
    src = os.path.join(HERE, "csrc", "mpc_witness_host_test.cpp")
    hdrs = [os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", f)
            for f in ("fe29.cuh", "fn_dev.cuh", "witness_dev.cuh", "mpc_witness_dev.cuh", "kernels.h", "fe29_consts.h")]
    if not os.path.exists(prog) or any(os.path.getmtime(f) > os.path.getmtime(prog) for f in [src] + hdrs):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                               "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", prog, src])
    return prog


def text_of(mo, p, q):
    """proof p of a model as party q holds it"""
    prog = mo.case.prog
    v, inputs, chi = mo.provers[p]
    rounds = mo.rounds
    lines = ["%x %x %x %x %x" % (prog.n, prog.m, prog.ninp, prog.nchi, len(rounds))]
    lines += ["%x" % x for x in chi]
    vq = [mc.md.unmont(b) for b in mc.md.cut(mo.v[q] or b"", 32)]
    iq = [mc.md.unmont(b) for b in mc.md.cut(mo.inputs[q] or b"", 32)]
    for k in range(3):
        lines += ["%x" % x for x in vq[(p * 3 + k) * prog.m:(p * 3 + k + 1) * prog.m]]
        lines += ["%x" % x for x in iq[(p * 3 + k) * 2 * prog.ninp:(p * 3 + k + 1) * 2 * prog.ninp]]
    pair = 0
    for op, arg, left, right in prog.gates:
        rows = [[(kind, idx, j, part) for kind, idx, coeff in row for j, part in enumerate(prog.parts(coeff)) if part is not None]
                for row in (left, right)]
        lines.append("%x %x %x %x" % (op, pair if op == mc.INPUT else arg, len(rows[0]), len(rows[1])))
        pair += op == mc.INPUT
        lines += ["%x %x %x %x" % t for row in rows for t in row]
    for r in rounds:
        lines.append("%x" % len(r["gates"]))
        lines += ["%x" % g for g in r["gates"]]
        lines += ["%x" % x for t in range(3) for k in range(3) for x in r["triples_ints"][p][q][t][k]]
        lines += ["%x" % x for de in range(2) for x in r["opened_ints"][p][de]]
    return lines


def want_of(mo, p, q):
    out = []
    for r in mo.rounds:
        for k in range(3):
            for s, i in enumerate(r["gates"]):
                pl = mo.ints[p][q]
                out.append((pl[0][k][i], pl[1][k][i], r["masked_ints"][q][p][0][k][s], r["masked_ints"][q][p][1][k][s], pl[2][k][i]) * 2)
    return out


@pytest.mark.parametrize("name", ["mpc_edges", "mpc_dag24", "range_inputs8"])
def test_program_prints_the_models_planes(exe, tmp_path, name):
    mo = mc.model(mc.case(name), 3)
    jobs = [(p, q) for p in range(3) for q in range(2)]
    lines = ["%x" % len(jobs)]
    for p, q in jobs:
        lines += text_of(mo, p, q)
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = [tuple(int(x, 16) for x in line.split()) for line in r.stdout.split("\n") if line]
    want = [row for p, q in jobs for row in want_of(mo, p, q)]
    assert len(got) == len(want)
    for at, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, at)


def test_program_refuses_what_the_library_would(exe, tmp_path):
    """the harness itself: a non-canonical value and a BIT gate end the program instead of being evaluated"""
    for text, code in (("1\n1 1 0 0 0\n%x\n1\n1\n0 0 0 0\n" % mc.N, 4), ("1\n1 1 0 0 0\n1\n1\n1\n2 0 0 0\n", 5)):
        path = tmp_path / "bad.txt"
        path.write_text(text)
        assert subprocess.run([exe, str(path)], capture_output=True, timeout=60).returncode == code
