"""The affine table builder of csrc/ec29.cuh (afftab_build: {1..8} P of the T points of a table lane, three levels, one shared
inversion per level) compiled for the CPU with -fsanitize=undefined (tests/csrc/afftab_host_test.cpp) and compared, entry by
entry, with the Python model's group law: random points, points with extreme coordinates, identity points at every position of
the lane, and the guard against a zero denominator."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pymodel as pm   # noqa: E402

P, N = pm.P, pm.N
R = 1 << 261                      # the Montgomery radix of fe29.cuh
SHAPES = (4, 8)


@pytest.fixture(scope="module")
def h():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libafftab_host.so")
    src = os.path.join(HERE, "csrc", "afftab_host_test.cpp")
    hdrs = [os.path.join(ROOT, "mpc_bulletproof_amd", "csrc", f) for f in ("fe29.cuh", "ec29.cuh", "fe29_consts.h")]
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fsanitize=undefined",
                               "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas", "-o", so, src])
    return C.CDLL(so)


def buf(b):
    return (C.c_uint8 * len(b)).from_buffer_copy(b)


def xy_bytes(x, y):
    return x.to_bytes(32, "little") + y.to_bytes(32, "little")


def build(h, T, pts, unchecked=False, skip=0):
    """-> (rc, rows[T][8] as model points, limbs[T][8][18], prefix slots used)"""
    raw = b"".join(pm.p2b(p) if not isinstance(p, bytes) else p for p in pts)
    out = (C.c_uint8 * (T * 8 * 64))()
    limbs = (C.c_int32 * (T * 8 * 18))()
    slots = C.c_int(0)
    rc = h.h29_afftab(T, buf(raw), 1 if unchecked else 0, skip, out, limbs, C.byref(slots))
    ob, lv = bytes(out), list(limbs)
    rows = [[ob[64 * (8 * j + e):64 * (8 * j + e + 1)] for e in range(8)] for j in range(T)]
    lm = [[lv[18 * (8 * j + e):18 * (8 * j + e + 1)] for e in range(8)] for j in range(T)]
    return rc, rows, lm, slots.value


def multiples(pt):
    out, acc = [], pm.INF
    for _ in range(8):
        acc = pm.pt_add(acc, pt)
        out.append(acc)
    return out


def check(h, T, pts, skip=0):
    rc, rows, limbs, slots = build(h, T, pts, skip=skip)
    assert rc == 0
    assert slots <= 4 * T                      # the staging a lane needs: the prefix products of the widest level
    for j, pt in enumerate(pts):
        want = multiples(pt)
        for e in range(8):
            assert pm.b2p(rows[j][e]) == want[e], (T, j, e)
            x, y = limbs[j][e][:9], limbs[j][e][9:]
            if pt is pm.INF:
                assert not any(x) and not any(y)     # a dead point's rows are all zero
                continue
            # T': lower limbs in [-8, 2^29 + 8); values inside the bounds stated in ec29.cuh (|x(kP)| <= (2k - 1) p, |y| <= 4p)
            for c in (x, y):
                assert all(-8 <= v < (1 << 29) + 8 for v in c[:8]), (T, j, e)
            vx = sum(v << (29 * t) for t, v in enumerate(x))
            vy = sum(v << (29 * t) for t, v in enumerate(y))
            assert abs(vx) <= (2 * (e + 1) - 1) * P and abs(vy) <= 4 * P, (T, j, e)


def curve_rhs(x):
    return (x * x * x + pm.CURVE_A * x + pm.CURVE_B) % P


def point_with_x(x):
    y = pm.fp_sqrt(curve_rhs(x % P))
    return None if y is None else (x % P, y)


# ---- roots of x^3 + x + (b - y^2) over F_p, for points with a chosen y: polynomials of degree < 3 as coefficient lists ----
def _pmulmod(a, b, f):
    """a b mod f, f monic of degree 3 (f = [c0, c1, c2])"""
    r = [0] * 5
    for i, ai in enumerate(a):
        for k, bk in enumerate(b):
            r[i + k] = (r[i + k] + ai * bk) % P
    for d in (4, 3):
        c = r[d]
        if c:
            for k in range(3):
                r[d - 3 + k] = (r[d - 3 + k] - c * f[k]) % P
            r[d] = 0
    return r[:3]


def _ppow(base, e, f):
    acc = [1, 0, 0]
    for bit in bin(e)[2:]:
        acc = _pmulmod(acc, acc, f)
        if bit == "1":
            acc = _pmulmod(acc, base, f)
    return acc


def _trim(p):
    p = [c % P for c in p]
    while p and p[-1] == 0:
        p.pop()
    return p


def _pmod(a, b):
    a, inv = _trim(a), pow(b[-1], -1, P)
    while len(a) >= len(b):
        c, s = a[-1] * inv % P, len(a) - len(b)
        a = _trim([(a[k] - c * b[k - s]) % P if k >= s else a[k] for k in range(len(a))])
    return a


def _pgcd(a, b):
    """monic gcd of two polynomials given as coefficient lists (low first); gcd(a, 0) = a"""
    a, b = _trim(a), _trim(b)
    while b:
        a, b = b, _pmod(a, b)
    inv = pow(a[-1], -1, P)
    return [c * inv % P for c in a]


def _pdiv_exact(g, d):
    """g / d for monic d dividing g"""
    q, quo = list(g), [0] * (len(g) - len(d) + 1)
    for k in range(len(g) - len(d), -1, -1):
        c = q[k + len(d) - 1]
        quo[k] = c
        for i, di in enumerate(d):
            q[k + i] = (q[k + i] - c * di) % P
    assert not any(q)
    return quo


def cubic_roots(c0):
    """roots of x^3 + x + c0 in F_p: gcd with x^p - x keeps the linear factors, random shifts split them"""
    f = [c0 % P, 1, 0]
    full = f + [1]
    xp = _ppow([0, 1, 0], P, f)
    roots, work, rnd = [], [_pgcd(full, [xp[0], xp[1] - 1, xp[2]])], random.Random(7)
    while work:
        g = work.pop()
        if len(g) == 2:
            roots.append(-g[0] % P)
        while len(g) > 2:
            t = _ppow([rnd.randrange(P), 1, 0], (P - 1) // 2, f)
            d = _pgcd(g, [t[0] - 1, t[1], t[2]])
            if 1 < len(d) < len(g):
                work += [d, _pdiv_exact(g, d)]
                break
    return roots


def point_with_y(y):
    for x in cubic_roots(pm.CURVE_B - y * y):
        assert curve_rhs(x) == y * y % P
        return (x, y % P)
    return None


def special_values():
    """1, p - 1, powers of two and values with zero low limbs -- as plain integers and as Montgomery images (the limbs the code sees)"""
    plain = [1, P - 1, 2, 1 << 29, 1 << 58, 1 << 116, 1 << 232, 1 << 250, 5 << 145, 3 << 203]
    ri = pow(R, -1, P)
    return plain + [v * ri % P for v in plain]


@pytest.fixture(scope="module")
def special_points():
    pts = []
    for v in special_values():
        for d in range(4):          # the value itself or, where no point has it, the nearest above with the same low limbs / bits
            a = point_with_x((v + (d << 240)) % P)
            if a:
                pts.append(a)
                break
        for d in range(4):
            b = point_with_y((v + (d << 240)) % P)
            if b:
                pts.append(b)
                break
    assert len(pts) >= 24 and all(pm.on_curve(p) for p in pts)
    return pts


@pytest.mark.parametrize("T", SHAPES)
def test_random_points(h, T):
    rnd = random.Random(1000 + T)
    for _ in range(6):
        check(h, T, [pm.pt_mul(rnd.randrange(1, N), pm.G) for _ in range(T)])
    # the same point in every slot, P beside -P and beside its own multiples: the points of a lane are independent of each other
    g3 = pm.pt_mul(3, pm.G)
    check(h, T, ([pm.G, pm.pt_neg(pm.G), g3, pm.pt_mul(2, pm.G)] * 2)[:T])
    check(h, T, [g3] * T)


@pytest.mark.parametrize("T", SHAPES)
def test_points_with_extreme_coordinates(h, T, special_points):
    pts = list(special_points)
    while len(pts) % T:
        pts.append(pm.G)
    for k in range(0, len(pts), T):
        check(h, T, pts[k:k + T])


@pytest.mark.parametrize("T", SHAPES)
def test_identity_points_at_every_position(h, T):
    rnd = random.Random(2000 + T)
    live = [pm.pt_mul(rnd.randrange(1, N), pm.G) for _ in range(T)]
    for j in range(T):                      # one identity at position j; one live point at position j
        one_dead = [pm.INF if k == j else live[k] for k in range(T)]
        one_live = [live[k] if k == j else pm.INF for k in range(T)]
        for pts, dead in ((one_dead, 1 << j), (one_live, ((1 << T) - 1) & ~(1 << j))):
            check(h, T, pts)                # identity known to this lane only
            check(h, T, pts, skip=dead)     # ... shared by the wave: passed over whole
            if bin(dead).count("1") > 1:
                check(h, T, pts, skip=dead & (dead - 1))   # some shared, one not
    for mask in (0b0101, 0b1010, 0b0110, (1 << T) - 1):
        pts = [pm.INF if (mask >> k) & 1 else live[k] for k in range(T)]
        check(h, T, pts)
        check(h, T, pts, skip=mask & ((1 << T) - 1))


@pytest.mark.parametrize("T", SHAPES)
def test_zero_denominator_is_reported_and_contained(h, T):
    """(x, 0) is on no curve of odd order: the doubling's denominator 2y is zero.  The builder reports it and the other points of
    the lane come out right."""
    rnd = random.Random(3000 + T)
    live = [pm.pt_mul(rnd.randrange(1, N), pm.G) for _ in range(T)]
    for j in (0, T // 2, T - 1):
        raw = [xy_bytes(12345, 0) if k == j else pm.p2b(live[k]) for k in range(T)]
        rc, rows, _, _ = build(h, T, raw, unchecked=True)
        assert rc == 1
        for k in range(T):
            if k != j:
                assert [pm.b2p(r) for r in rows[k]] == multiples(live[k]), (T, j, k)
    rc, rows, _, _ = build(h, T, [pm.p2b(p) for p in live], unchecked=True)
    assert rc == 0 and all([pm.b2p(r) for r in rows[k]] == multiples(live[k]) for k in range(T))
