"""mul2 of csrc/fe29.cuh, (a b + c d) / R with ONE Montgomery reduction, and the point additions of csrc/ec29.cuh that take their
Y through it, compiled for the CPU with -fsanitize=undefined (tests/csrc/mul2_host_test.cpp, a program of its own run as a child
process) and checked against Python big integers / the Python model on the operands of tests/fused_product_cases.py.  A signed
overflow in any 64-bit column sum aborts the program: the run over operands with every limb at +-(2^29 + 8) is the bound's proof."""
import os
import subprocess

import pytest

import fused_product_cases as fc

pm = fc.pm
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def prog():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "mul2_host_test")
    src = os.path.join(HERE, "csrc", "mul2_host_test.cpp")
    hdrs = [os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", f) for f in ("fe29.cuh", "ec29.cuh", "fe29_consts.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                               "-Wno-unknown-pragmas", "-o", exe, src])

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])       # UBSan's report and abort land here
        got = r.stdout.split("\n")[:-1]
        assert len(got) == len(lines)
        return got
    return run


def _flat(*vs):
    return " ".join(str(x) for v in vs for x in v)


def test_mul2_on_raw_limbs_at_the_contract_bounds(prog):
    cases = fc.mul2_cases()
    got = prog(["M " + _flat(*case) for _, case in cases])
    for (name, case), g in zip(cases, got):
        assert int(g, 16) == fc.want(case), name
    by_name = dict(cases)
    assert all(fc.want(by_name[n]) == 0 for n in by_name if n.startswith("zero"))
    assert fc.want(by_name["one: R * 1"]) == fc.want(by_name["one: split"]) == 1
    assert fc.want(by_name["minus one: R * -1"]) == fc.want(by_name["minus one: split"]) == fc.P - 1
    # the worst case does reach the column maximum (column 7: 8 + 8 terms of lower limbs, each B^2), and the header's bound for a
    # column of 9 + 9 such terms, the reduction terms and the carry fits the accumulator
    hi = by_name["columns at +max"]
    col7 = sum(hi[0][j] * hi[1][7 - j] for j in range(8)) + sum(hi[2][j] * hi[3][7 - j] for j in range(8))
    assert col7 == 16 * fc.B ** 2 and 18 * fc.B ** 2 + (1 << 52) + (1 << 34) < 1 << 63


def test_mul2_with_a_zero_second_product_equals_mul(prog):
    cases = fc.mul_edge_cases()
    got = prog(["E " + _flat(a, b, d) for a, b, d in cases])
    for (a, b, d), g in zip(cases, got):
        fused, plain = (int(x, 16) for x in g.split())
        assert fused == plain == fc.value(a) * fc.value(b) * fc.RINV % fc.P, (a, b)


def test_changed_additions_on_the_point_table_including_exceptional_cases(prog):
    pts = fc.points(6)
    reqs = [(op, a, b) for a in pts for b in pts for op in fc.POINT_OPS]
    got = prog(["P %d %s %s" % (op, pm.p2b(a).hex(), pm.p2b(b).hex()) for op, a, b in reqs])
    for (op, a, b), g in zip(reqs, got):
        rc, out = g.split()
        if op in (4, 5) and b is pm.INF:
            assert int(rc) == -3
            continue
        assert int(rc) == 0 and pm.b2p(bytes.fromhex(out)) == pm.pt_add(a, b), (op, a, b)
