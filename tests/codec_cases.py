"""Crafted inputs for the point codec's square root (csrc/fe29_sqrt.cuh, csrc/k_codec.hip).  Test infrastructure, no GPU:
tests/test_codec_cases.py checks it against the model, tests/test_gpu_codec_crafted.py, tests/test_gpu_arith.py and
tests/test_gpu_ark_edges.py drive the kernels with it.

fp_sqrt finds e' with a^t = c^(e') (p - 1 = 2^192 t, c = 3^t) as 24 eight-bit digits, digit 0 lowest, by a recursive
Pohlig-Hellman that splits the digit range 12 | 12, 6 | 6, 3 | 3, 1 | 2, 1 | 1, and multiplies a^((t+1)/2) by c^(-e'/2) digit by
digit, bit 0 of digit j + 1 carried into bit 7 of digit j.  For a random a all 24 digits are uniform.  Here they are chosen:

  digits    a = c^e h with e = e' / t mod 2^192 and h of odd order has exactly the digits e'; an odd e' is a non-residue
  sign      the curve points whose y lies next to (p - 1) / 2, (p + 1) / 2, 1 and p - 1: the comparison that picks the root
  xrange    x at 0, 1, 2, p - 3, p - 2, p - 1, the non-canonical x at and past p, and x = p - 1 under every flag pair

Decompression takes x, not a = x^3 + x + b, so a chosen a needs a root of the cubic X^3 + X + (b - a): gcd(X^p - X, f), then
equal-degree splitting with (X + d)^((p - 1) / 2) - 1.  About two targets in three have one; a digit pattern draws h from a seeded
generator until its a has (at most DRAWS times; build().skipped lists a pattern that found none and must stay empty).

An encoding is 32 bytes: x little-endian, bit 7 of byte 31 = "y is the larger of (y, -y)", bit 6 = identity (oracle/pymodel.py
point_decompress is the reference for every verdict)."""
import collections
import functools
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import pymodel as pm  # noqa: E402

P, B = pm.P, pm.CURVE_B
assert pm.CURVE_A == 1
S2 = 192                              # 2-adicity of p - 1
T = (P - 1) >> S2
C_GEN = pow(3, T, P)                  # generates the 2-Sylow subgroup
T_INV = pow(T, -1, 1 << S2)
HALF = (P - 1) // 2
DRAWS = 20
ND = 24


# ------------------------------------------------------------------ polynomials over F_p, coefficient lists low -> high
def _trim(u):
    u = [c % P for c in u]
    while u and u[-1] == 0:
        u.pop()
    return u


def _divmod(u, m):
    """-> (quotient, remainder) of u by m (m not zero)"""
    u, m = _trim(u), _trim(m)
    inv = 1 if m[-1] == 1 else pow(m[-1], -1, P)
    q = [0] * max(len(u) - len(m) + 1, 0)
    while len(u) >= len(m):
        c, s = u[-1] * inv % P, len(u) - len(m)
        q[s] = c
        for i, mc in enumerate(m):
            u[s + i] = (u[s + i] - c * mc) % P
        u = _trim(u)
    return q, u


def _mulmod(u, v, m):
    r = [0] * (len(u) + len(v) - 1) if u and v else []
    for i, a in enumerate(u):
        for j, b in enumerate(v):
            r[i + j] += a * b
    return _divmod(r, m)[1]


def _powmod(base, e, m):
    acc, base = [1], _divmod(base, m)[1]
    for bit in bin(e)[2:]:
        acc = _mulmod(acc, acc, m)
        if bit == "1":
            acc = _mulmod(acc, base, m)
    return acc


def _sub(u, v):
    n = max(len(u), len(v))
    return _trim([(u[i] if i < len(u) else 0) - (v[i] if i < len(v) else 0) for i in range(n)])


def _gcd(u, v):
    u, v = _trim(u), _trim(v)
    while v:
        u, v = v, _divmod(u, v)[1]
    inv = pow(u[-1], -1, P)
    return [c * inv % P for c in u]


def _roots_of_split(g, rnd):
    """all roots of a monic g that is a product of distinct linear factors"""
    if len(g) == 1:
        return []
    if len(g) == 2:
        return [(-g[0]) % P]
    while True:
        w = _sub(_powmod([rnd.randrange(P), 1], HALF, g), [1])
        h = _gcd(g, w) if w else g
        if 1 < len(h) < len(g):
            return _roots_of_split(h, rnd) + _roots_of_split(_divmod(g, h)[0], rnd)


def cubic_roots(a, rnd):
    """every x in F_p with x^3 + x + b = a, ascending"""
    f = [(B - a) % P, 1, 0, 1]
    w = _sub(_powmod([0, 1], P, f), [0, 1])           # X^p - X mod f
    g = _gcd(f, w) if w else f                          # the product of f's linear factors
    xs = sorted(_roots_of_split(g, rnd))
    assert all((x * x * x + x + B - a) % P == 0 for x in xs)
    return xs


def rhs(x):
    return (x * x * x + x + B) % P


# ------------------------------------------------------------------ encodings
FLAG_BITS = {"00": 0, "01": 0x40, "10": 0x80, "11": 0xC0}


def encode(x, flags):
    """x < 2^254 with the two flag bits named as the pair (bit 7, bit 6)"""
    assert 0 <= x < 1 << 254
    b = bytearray(x.to_bytes(32, "little"))
    b[31] |= FLAG_BITS[flags]
    return bytes(b)


def model_decode(enc):
    """-> (ok, 64 bytes) as bpgpu_points_decompress reports them: zeros where the model raises, and for the identity"""
    try:
        return 1, pm.p2b(pm.point_decompress(enc))
    except pm.FormatError:
        return 0, bytes(64)


def digits_of(e):
    return list(e.to_bytes(ND, "little"))


def digit_patterns():
    """-> [(name, e')]: the 24 digits of the discrete logarithm, as an integer"""
    full = (1 << S2) - 1
    pats = [("zero", 0), ("top_bit", 1 << 191), ("all_ff", full), ("all_ff_but_bit0", full - 1),
            ("80_every", int("80" * ND, 16)), ("01_every", int("01" * ND, 16)), ("0100_repeated", int("0100" * (ND // 2), 16)),
            ("ff00_repeated", int("ff00" * (ND // 2), 16)), ("00ff_repeated", int("00ff" * (ND // 2), 16))]
    for j in (0, 1, 11, 12, 22, 23):
        for d in (0x01, 0x02, 0x80, 0xFF):                 # 0x01 at j >= 1 is the carry into digit j - 1
            pats.append((f"single_{d:02x}_at_{j}", d << (8 * j)))
    # the split points of the recursion's first four levels: 12 | 12, 6 | 6, 3 | 3, 1 | 2
    for s in (12, 6, 18, 3, 9, 15, 21, 1, 4, 7, 10, 13, 16, 19, 22):
        low = (1 << (8 * s)) - 1
        pats.append((f"ff_below_{s}", low))
        pats.append((f"ff_from_{s}", full - low))
    assert len({n for n, _ in pats}) == len(pats)      # (ff_below_1 repeats single_ff_at_0 with another odd-order part)
    return pats


SINGLE_DIGIT = "single_"          # name prefix of the family a fresh context decodes first

Case = collections.namedtuple("Case", "family name enc kind a")
"""kind: what the family intends the model to say -- valid, identity, nonresidue (x canonical and off the curve) or noncanonical
(x >= p or both flag bits).  a: the square root's argument for x < p, else None."""
Built = collections.namedtuple("Built", "cases skipped sign_points x_points sqrt_args")


@functools.lru_cache(maxsize=None)
def build():
    rnd = random.Random(0xC0DEC)
    cases, skipped, sqrt_args = [], [], []

    # ---- digits
    for name, e1 in digit_patterns():
        e = e1 * T_INV % (1 << S2)
        for _ in range(DRAWS):
            h = pow(rnd.randrange(2, P), 1 << S2, P)       # odd order
            a = pow(C_GEN, e, P) * h % P
            xs = cubic_roots(a, rnd)
            if xs:
                break
        else:
            skipped.append(name)
            continue
        assert pow(a, T, P) == pow(C_GEN, e1, P)
        assert pow(h, T, P) == 1 and (e1 != 0 or pow(a, T, P) == 1)
        x = xs[0]
        kind = "nonresidue" if e1 & 1 else "valid"
        sqrt_args.append(("digits", name, a))
        for fl in ("00", "10"):
            cases.append(Case("digits", f"{name}/{fl}", encode(x, fl), kind, a))
        cases.append(Case("digits", f"{name}/01", encode(x, "01"), "identity", a))

    # ---- sign: the y next to the boundary of "y is the larger of (y, -y)" and next to 0 that have a point
    sign_points = []
    for name, y0, step, want_off in (("below_half", HALF, -1, 1), ("above_half", HALF + 1, 1, 1), ("above_zero", 1, 1, 1),
                                     ("below_p", P - 1, -1, 1)):
        off = 0
        while not cubic_roots((y0 + off * step) ** 2 % P, rnd):
            off += 1
            assert off <= 8, name
        assert off == want_off, (name, off)
        y = y0 + off * step
        sqrt_args.append(("sign", name, y * y % P))
        for i, x in enumerate(cubic_roots(y * y % P, rnd)):
            assert pm.on_curve((x, y))
            sign_points.append((x, y))
            for fl in ("00", "10"):
                cases.append(Case("sign", f"{name}/x{i}/{fl}", encode(x, fl), "valid", y * y % P))

    # ---- xrange
    x_points = []
    for name, x, on in (("0", 0, False), ("1", 1, True), ("2", 2, True), ("p-3", P - 3, False), ("p-2", P - 2, True), ("p-1", P - 1, True)):
        y = pm.fp_sqrt(rhs(x))
        assert (y is not None) == on, name
        sqrt_args.append(("xrange", name, rhs(x)))
        if on:
            x_points += [(x, y), (x, P - y)]
        for fl in ("00", "10"):
            cases.append(Case("xrange", f"x={name}/{fl}", encode(x, fl), "valid" if on else "nonresidue", rhs(x)))
    for name, x in (("p", P), ("p+1", P + 1), ("2^252", 1 << 252), ("2^254-1", (1 << 254) - 1)):
        for fl in ("00", "10", "01"):                      # (x >= p is no identity either: p itself would pass for x = 0)
            cases.append(Case("xrange", f"x={name}/{fl}", encode(x, fl), "noncanonical", None))
    cases.append(Case("xrange", "x=p-1/01", encode(P - 1, "01"), "identity", rhs(P - 1)))
    cases.append(Case("xrange", "x=p-1/11", encode(P - 1, "11"), "noncanonical", rhs(P - 1)))
    return Built(tuple(cases), tuple(skipped), tuple(sign_points), tuple(x_points), tuple(sqrt_args))


def summary():
    """family -> (encodings, encodings the model accepts, square-root arguments, residues among them)"""
    b = build()
    out = {}
    for fam in ("digits", "sign", "xrange"):
        cs = [c for c in b.cases if c.family == fam]
        args = [a for f, _, a in b.sqrt_args if f == fam]
        out[fam] = (len(cs), sum(model_decode(c.enc)[0] for c in cs), len(args), sum(pm.fp_sqrt(a) is not None for a in args))
    return out
