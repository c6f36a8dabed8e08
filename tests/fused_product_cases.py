"""Operands for mul2 of csrc/fe29.cuh, (a b + c d) / R with one reduction, as RAW limb vectors (9 x int32, lower limbs of magnitude
<= B = 2^29 + 8: the header's contract), and the point table of the group-law forms that use it.  Test infrastructure, pure
Python on big integers; tests/test_fused_products_cpu.py feeds them to the CPU build of the headers (UBSan on every 64-bit column
sum), tests/test_gpu_fused_products.py to the device's asm MAD chains.  The expected value is value(a) value(b) + value(c) value(d)
over R modulo p in Python integers, never another build of the code under test."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pymodel as pm   # noqa: E402

P, N = pm.P, pm.N
NL, LB = 9, 29
R = 1 << (NL * LB)
RINV = pow(R, -1, P)
B = (1 << LB) + 8            # the largest magnitude of a lower limb
TOP = (1 << 24) - 2          # a top limb: the limbs' value stays below 2^256 with every lower limb at +-B


def value(v):
    return sum(x << (LB * j) for j, x in enumerate(v))


def limbs(x):
    """canonical limbs of 0 <= x < 2^261"""
    return [(x >> (LB * j)) & ((1 << LB) - 1) for j in range(NL)]


def want(case):
    a, b, c, d = case
    return (value(a) * value(b) + value(c) * value(d)) * RINV % P


def neg(v):
    return [-x for x in v]


def edge_values(m=P):
    """the edge list of tests/test_device_arith_cpu.py"""
    return [x % m for x in (0, 1, 2, m - 1, m - 2, (m + 1) // 2, 2**128 - 1, 2**250)]


def mul2_cases(count=100, seed=5):
    """[(name, (a, b, c, d))]"""
    rnd = random.Random(seed)
    hi, lo = [B] * 8 + [TOP], [-B] * 8 + [-TOP]
    out = [("all +B", (hi, hi, hi, hi)), ("all -B", (lo, lo, lo, lo)),
           # same sign: every term of every one of the 17 columns at its positive / negative maximum
           ("columns at +max", (hi, hi, lo, lo)), ("columns at -max", (hi, lo, lo, hi)),
           # mixed signs: the two products at opposite maxima
           ("max minus max", (hi, hi, hi, lo)), ("minus max plus max", (lo, hi, lo, lo))]
    # alternating signs inside a column, and one product at its maximum against lower limbs of one sign only
    alt = [B if j % 2 == 0 else -B for j in range(8)] + [TOP]
    out += [("alternating", (alt, alt, neg(alt), alt)), ("alternating against +B", (alt, hi, hi, neg(alt))),
            ("lower limbs only", ([B] * 8 + [0], [B] * 8 + [0], [B] * 8 + [0], [B] * 8 + [0]))]
    # results that must be 0 and +-1
    x, y = limbs(rnd.randrange(P)), limbs(rnd.randrange(P))
    one, zero, r_mod = [1] + [0] * 8, [0] * 9, limbs(R % P)
    t = rnd.randrange(P)
    out += [("zero: ab = -cd", (x, y, neg(x), y)), ("zero: ab = -cd, d negated", (x, y, x, neg(y))), ("zero: all zero", (zero, zero, zero, zero)),
            ("one: R * 1", (r_mod, one, zero, zero)), ("minus one: R * -1", (zero, hi, r_mod, neg(one))),
            ("one: split", (one, limbs((R - t) % P), one, limbs(t))), ("minus one: split", (neg(one), limbs((R - t) % P), limbs(t), neg(one)))]
    for i in range(count):
        out.append(("canonical %d" % i, tuple(limbs(rnd.randrange(P)) for _ in range(4))))

    def wide():
        return [rnd.choice([-B, B, 0, rnd.randint(-B, B)]) for _ in range(8)] + [rnd.randint(-TOP, TOP)]
    for i in range(count):
        out.append(("raw %d" % i, (wide(), wide(), wide(), wide())))
    # the operands of the group law: un-normalised differences of a tight and a T' value against tight ones
    for i in range(count // 2):
        tight = [limbs(rnd.randrange(P)) for _ in range(4)]
        tp = [[rnd.choice([-8, (1 << LB) + 7, rnd.randint(-8, (1 << LB) + 7)]) for _ in range(8)] + [rnd.randint(0, 1 << 22)] for _ in range(3)]
        out.append(("differences %d" % i, ([u - v for u, v in zip(tight[0], tp[0])], [u - v for u, v in zip(tight[1], tp[1])], neg(tp[2]), tight[2])))
    for name, case in out:
        assert all(abs(x) <= B for v in case for x in v[:8]) and all(abs(value(v)) < 1 << 256 for v in case), name
    return out


def mul_edge_cases():
    """(a, b, d): a b + 0 d must equal mul(a, b), for the edge list squared and d at the bounds"""
    e = edge_values()
    ds = [[B] * 8 + [TOP], [-B] * 8 + [-TOP], limbs(P - 1)]
    return [(limbs(x), limbs(y), ds[(i + j) % 3]) for i, x in enumerate(e) for j, y in enumerate(e)]


def points(n_random, seed=31):
    rnd = random.Random(seed)
    return [pm.INF, pm.G, pm.pt_neg(pm.G), pm.pt_mul(2, pm.G)] + [pm.pt_mul(rnd.randrange(1, N), pm.G) for _ in range(n_random)]


# the group-law forms whose hot path takes mul2 (the numbering of tests/csrc/mul2_host_test.cpp and mul2_gpu_test.hip)
#   0  jac_madd(a, b)            1  jac_add, both operands rescaled to non-trivial Z     3  ((identity + a) + b) by xyzz_madd
#   4  xyzz_madd_nzq into a rescaled accumulator (b != identity)      5  jac_madd_nzq into a rescaled accumulator (b != identity)
POINT_OPS = (0, 1, 3, 4, 5)
