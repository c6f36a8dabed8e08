"""The accumulator walk of the table kernels (csrc/ec29.cuh: xyzz_inf, fp_sign_nr, xyzz_madd_nzq), compiled for the CPU with
-fsanitize=undefined (tests/csrc/walk_host_test.cpp, a program of its own run as a child process) and checked step by step against
the Python model (oracle/pymodel.py).

An accumulator starts as xyzz_inf(), whose all-zero X sends it through the one-limb filter into the guarded branch of
xyzz_madd_nzq; an addend whose digit is negative arrives with y negated limb by limb, as an operand of one product.  The program
asserts after every addition that the four stored coordinates are T / T' and, through the operand hook of ec29.cuh, that every
operand of every product of the group law is inside the contract of fe29.cuh; UBSan aborts it on a signed overflow in a column."""
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pymodel as pm   # noqa: E402

N = pm.N


@pytest.fixture(scope="module")
def prog():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "walk_host_test")
    src = os.path.join(HERE, "csrc", "walk_host_test.cpp")
    hdrs = [os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", f) for f in ("fe29.cuh", "ec29.cuh", "fe29_consts.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                               "-Wno-unknown-pragmas", "-o", exe, src])

    def run(walks):
        """walks: lists of (digit sign, point).  Returns per walk the accumulator after every addend and the count of products that
        took a limbwise-negated operand."""
        lines = ["W %d %s" % (len(w), " ".join("%d %s" % (d, pm.p2b(p).hex()) for d, p in w)) for w in walks]
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])       # a bound, UBSan's report and abort land here
        got = r.stdout.split("\n")[:-1]
        assert len(got) == len(walks)
        res = []
        for g, w in zip(got, walks):
            toks = g.split()
            assert len(toks) == len(w) + 1
            res.append(([pm.b2p(bytes.fromhex(t)) for t in toks[:-1]], int(toks[-1])))
        return res
    return run


def _model(walk):
    acc, out = pm.INF, []
    for d, p in walk:
        acc = pm.pt_add(acc, p if d > 0 else pm.pt_neg(p))
        out.append(acc)
    return out


def _points(n, seed):
    rnd = random.Random(seed)
    return [pm.pt_mul(rnd.randrange(1, N), pm.G) for _ in range(n)]


def test_walks_from_the_identity_over_both_signs_into_cancellation(prog):
    P, Q, R, S = _points(4, 11)
    walks = {
        "one positive": [(1, P)],
        "one negative": [(-1, P)],                                     # the fill stores -y behind a carry pass
        "positive chain": [(1, P), (1, Q), (1, R), (1, S)],
        "negative chain": [(-1, P), (-1, Q), (-1, R), (-1, S)],
        "mixed chain": [(1, P), (-1, Q), (-1, R), (1, S), (-1, P)],
        "P - P then on": [(1, P), (-1, P), (1, Q), (-1, R)],           # back at the identity in mid-walk, filled anew
        "-P + P then on": [(-1, P), (1, P), (-1, Q), (1, R)],
        "P + P": [(1, P), (1, P), (1, Q)],                             # the out-of-line doubling
        "-P - P": [(-1, P), (-1, P), (-1, Q)],                         # ... with the addend negated limb by limb
        "cancel twice": [(1, P), (-1, P), (-1, Q), (1, Q), (1, R)],
        "generator": [(1, pm.G), (-1, pm.G), (-1, pm.G), (-1, pm.G)],
    }
    # deep cancellation and doubling: the addend is the accumulator's own value (or its negative) after a chain, so the accumulator
    # that meets it has grown ZZ, ZZZ
    chain = [(1, P), (-1, Q), (1, R)]
    total = _model(chain)[-1]
    walks["chain minus its sum"] = chain + [(-1, total), (1, S)]
    walks["chain minus its negated sum"] = chain + [(1, pm.pt_neg(total)), (-1, S)]
    walks["chain plus its sum"] = chain + [(1, total), (1, S)]
    walks["chain plus its sum, negative digit"] = chain + [(-1, pm.pt_neg(total)), (1, S)]
    rnd = random.Random(12)
    pts = _points(12, 13)
    for i in range(8):
        walks["random %d" % i] = [(rnd.choice((1, -1)), rnd.choice(pts)) for _ in range(24)]      # repeats: doublings and cancellations by chance
    names = list(walks)
    got = prog([walks[nm] for nm in names])
    for nm, (accs, negated) in zip(names, got):
        assert accs == _model(walks[nm]), nm
        # a walk with a negative digit past its first addend did multiply by a limbwise-negated operand (q.y * ZZZ)
        if any(d < 0 for d, _ in walks[nm][1:]):
            assert negated > 0, nm
    assert _model(walks["P - P then on"])[1] is pm.INF or _model(walks["P - P then on"])[1] == pm.INF
    assert _model(walks["chain minus its sum"])[3] == pm.INF
