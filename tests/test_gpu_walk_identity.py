"""The table walks' accumulators at their identity, on scalars built digit by digit, bit for bit against the CPU oracle.

An accumulator of a table walk (csrc/ec29.cuh: Xyzz) starts as the identity, takes its first row in the guarded branch of
xyzz_madd_nzq (the all-zero X of xyzz_inf() trips the one-limb filter), can return to the identity in mid-run (P then -P) and
can meet its own value (P then P: the out-of-line doubling).  A negative digit hands the row's y over negated limb by limb; where
that row FILLS an accumulator the stored Y is carried first.  The cases:

  generator walk   csrc/fixed_body.cuh through the harness tests/csrc/walk_gpu_test.hip (the verifier feeds these bodies scalars
                   of its transcript only): tables of width 8 and 20 over [B, B~, G_0..G_3, H_0..H_3] =
                   [0, P, -P, Q, 0, 0, R, R, S, 0] (0 = the identity), batches of 1, 65 and 257 proofs, runs of 1, 3 and 6
                   generators per wave (fixed_chunk_body) and 32 lanes per proof (fixed_small_body).  The proofs of a wave take
                   the patterns of _patterns() in turn, so its lanes mix them.
  window walk      k_verify_windows through bpgpu_msm with 1, 2 and 17 points

Every partial sum, every sum of partials and every MSM is compared with the oracle's scalar multiplication of the known discrete
logarithm; nothing is compared with another GPU result.  Run with `-m gpu` on an MI355X."""
import ctypes as C
import os
import random

import pytest

import oracle_lib as o
import window_digits as wd

pytestmark = pytest.mark.gpu
N = o.N
ZERO = bytes(64)
HERE = os.path.dirname(os.path.abspath(__file__))

KP, KQ, KR, KS = (0x1D2C3B4A59687766554433221100FFEEDDCCBBAA998877, 0x7A6B5C4D3E2F10213243546576879809A0B1C2D3E4F5,
                  0x5DEECE66D1234567890ABCDEF0FEDCBA9876543210F00DFACE, 0x3C0FFEE0DDBA11CAFEF00D5EED1E55ACCE55ED)
# discrete logarithms of the ten generators; 0 = the identity, whose scalar must not matter
KS10 = [0, KP, N - KP, KQ, 0, 0, KR, KR, KS, 0]
RUNS = (1, 3, 6)


def _mulG(k):
    return o.point_mul(o.s2b(k), o.generator()) if k % N else ZERO


# ------------------------------------------------------------------ the generator walk
def _one(c, w, d):
    """the scalar whose digit in window w is d (a negative d with its +1 in window w + 1) and every other digit zero"""
    return (d << (c * w)) + ((1 << (c * (w + 1))) if d < 0 else 0)


def _patterns(c):
    """name -> 10 scalars.  Generators 0, 4, 5, 9 are the identity and get non-zero scalars in every pattern but `zero`."""
    W, half = wd.windows(c), 1 << (c - 1)
    rnd = random.Random(4200 + c)
    rs = lambda: rnd.randrange(1, N)      # noqa: E731
    top = wd.top_digit(c)
    out = {}
    out["zero"] = [0] * 10
    # zero digits in the first three windows of every scalar: an accumulator is first filled in mid-generator
    out["late_start"] = [(rs() >> (3 * c)) << (3 * c) for _ in range(10)]
    assert all(wd.digits(s, c)[:3] == [0, 0, 0] for s in out["late_start"])
    # only the top window: one addition per generator, the last pair of its walk
    out["top_only"] = [(1 + i % top) << (c * (W - 1)) for i in range(10)]
    assert all(s < N and wd.digits(s, c)[:W - 1] == [0] * (W - 1) for s in out["top_only"])
    out["n_minus_1"] = [N - 1] * 10
    out["n_minus_2"] = [N - 2] * 10
    # equal scalars on P and -P: the accumulator is the identity again after -P's last window and is filled anew by Q
    a = rs()
    out["cancel"] = [rs(), a, a, rs(), rs(), rs(), rs(), rs(), rs(), rs()]
    # one row on R and the same row on the second R: the accumulator meets itself (P = R = 0: the out-of-line doubling)
    out["double"] = [rs(), 0, 0, 0, rs(), rs(), _one(c, 1, half - 1), _one(c, 1, half - 1), rs(), rs()]
    out["double_top"] = [rs(), 0, 0, 0, rs(), rs(), top << (c * (W - 1)), top << (c * (W - 1)), 0, rs()]
    # row d of P, then digit -d on -P: the same row arrives negated limb by limb at an accumulator that holds it -- a doubling with
    # a negative digit -- and window w + 1 of -P goes on from there
    out["double_negative"] = [rs(), _one(c, 2, half - 1), _one(c, 2, -(half - 1)), rs(), rs(), rs(), 0, 0, 0, rs()]
    # the first addition of the walk carries a negative digit: the stored Y of the fill is -y, carried
    out["negative_fill"] = [rs(), (1 << c) - 1, 0, 0, rs(), rs(), _one(c, 0, -half), 0, N - 1, rs()]
    assert wd.digits((1 << c) - 1, c)[:2] == [-1, 1]
    # identity generators alone carry scalars: every partial sum is the identity
    out["identities_only"] = [N - 1, 0, 0, 0, rs(), N - 2, 0, 0, 0, 1]
    out["random"] = [rs() for _ in range(10)]
    out["random2"] = [rs() for _ in range(10)]
    assert all(0 <= s < N for v in out.values() for s in v)
    return out


_WANT = {}


def _want(scalars, g0, g1):
    """the oracle's point for generators [g0, g1) of one proof: computed once per distinct (scalars, range)"""
    key = (tuple(scalars[g0:g1]), g0)
    if key not in _WANT:
        _WANT[key] = _mulG(sum(s * k for s, k in zip(scalars[g0:g1], KS10[g0:g1])) % N)
    return _WANT[key]


class _Walk:
    def __init__(self):
        path = os.path.join(HERE, "csrc", "libwalk_gpu.so")
        assert os.path.exists(path), "tests/csrc/libwalk_gpu.so is missing: __graft_entry__.build() makes it"
        self.lib = C.CDLL(path)
        self.lib.wg_table_create.restype = C.c_void_p
        self.lib.wg_table_create.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        self.lib.wg_table_destroy.argtypes = [C.c_void_p]
        self.lib.wg_chunk_walk.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint, C.c_char_p, C.POINTER(C.c_int), C.c_char_p]
        self.lib.wg_small_walk.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p]
        self.tables = {}

    def table(self, c):
        if c not in self.tables:
            gens = b"".join(_mulG(k) for k in KS10)
            assert [gens[64 * i:64 * i + 64] == ZERO for i in range(10)] == [k == 0 for k in KS10]
            t = self.lib.wg_table_create(c, gens, 10)
            assert t, "no table (no device, no memory or a malformed generator)"
            self.tables[c] = t
        return self.tables[c]

    def chunk_walk(self, c, proofs, run):
        nb, chunks = len(proofs), -(-10 // run)
        parts, sums = C.create_string_buffer(64 * nb * chunks), C.create_string_buffer(64 * nb)
        inf = (C.c_int * (nb * chunks))()
        rc = self.lib.wg_chunk_walk(self.table(c), o.scalars([s for p in proofs for s in p]), nb, run, parts, inf, sums)
        assert rc == 0, rc
        return parts.raw, list(inf), sums.raw

    def small_walk(self, c, proofs):
        out = C.create_string_buffer(64 * len(proofs))
        rc = self.lib.wg_small_walk(self.table(c), o.scalars([s for p in proofs for s in p]), len(proofs), out)
        assert rc == 0, rc
        return out.raw

    def close(self):
        for t in self.tables.values():
            self.lib.wg_table_destroy(t)


@pytest.fixture(scope="module")
def walk():
    w = _Walk()
    yield w
    w.close()


def _check_chunks(walk, c, names, proofs, run, tag):
    parts, inf, sums = walk.chunk_walk(c, proofs, run)
    chunks = -(-10 // run)
    for i, (nm, sc) in enumerate(zip(names, proofs)):
        for q in range(chunks):
            want = _want(sc, q * run, min(10, q * run + run))
            k = i * chunks + q
            where = "%s proof %d (%s) chunk %d" % (tag, i, nm, q)
            assert parts[64 * k:64 * k + 64] == want, where
            if nm in ("zero", "identities_only"):
                assert want == ZERO and inf[k] == 1, where      # nothing was added: the stored partial is the identity, Z = 0 limb by limb
        assert sums[64 * i:64 * i + 64] == _want(sc, 0, 10), "%s proof %d (%s) sum of partials" % (tag, i, nm)


@pytest.mark.parametrize("nb", [1, 65, 257])
@pytest.mark.parametrize("c", [8, 20])
def test_generator_walk_from_into_and_through_the_identity(walk, c, nb):
    """fixed_chunk_body<C, 1> in runs of 1, 3 and 6 generators over [0, P, -P, Q, 0, 0, R, R, S, 0]: identity generators first in a
    run (0), in its middle (4, 5: runs [3, 4, 5] and [0..5]) and last (5 of [3, 4, 5], 9 of [6..9]), alone in a run of 1; -P right
    after P and R right after R inside the runs [0, 1, 2], [0..5], [6, 7, 8] and [6..9].  nb = 1: a call per pattern; 65 and 257:
    the patterns in turn, a proof per lane, two and five waves per run of generators with the last one a single lane."""
    pats = _patterns(c)
    names = list(pats)
    assert _want(pats["cancel"], 1, 3) == ZERO and _want(pats["cancel"], 0, 6) == _mulG(pats["cancel"][3] * KQ)
    assert _want(pats["double"], 6, 8) == _mulG(2 * pats["double"][6] * KR) != ZERO
    assert _want(pats["double_negative"], 1, 3) == _mulG((2 * pats["double_negative"][1] - (1 << (3 * c))) * KP) != ZERO
    for run in RUNS:
        if nb == 1:
            for nm in names:
                _check_chunks(walk, c, [nm], [pats[nm]], run, "c = %d run %d nb 1" % (c, run))
        else:
            seq = [names[i % len(names)] for i in range(nb)]
            _check_chunks(walk, c, seq, [pats[nm] for nm in seq], run, "c = %d run %d nb %d" % (c, run, nb))


@pytest.mark.parametrize("c", [8, 20])
def test_generator_walk_on_lanes_per_proof(walk, c):
    """fixed_small_body<C, 32>: lane l of a proof takes pairs l, l + 32, ... of the 10 W, so its first row, a cancellation and a
    doubling fall where the stride puts them; the lanes are added by the shuffle butterfly.  65 proofs, the patterns in turn."""
    pats = _patterns(c)
    names = list(pats)
    seq = [names[i % len(names)] for i in range(65)]
    got = walk.small_walk(c, [pats[nm] for nm in seq])
    for i, nm in enumerate(seq):
        assert got[64 * i:64 * i + 64] == _want(pats[nm], 0, 10), "c = %d proof %d (%s)" % (c, i, nm)


# ------------------------------------------------------------------ the window walk
@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


def _neg(pt):
    return pt[:32] + ((o.P - int.from_bytes(pt[32:], "little")) % o.P).to_bytes(32, "little")


def _window_cases(n):
    """[(name, scalars, points as a list of 64-byte strings)]: 4-bit digits, lane = window, the points of an MSM one after another"""
    rnd = random.Random(8800 + n)
    pts = [o.gens("G", 17)[64 * i:64 * i + 64] for i in range(17)][:n]
    rs = lambda: rnd.randrange(1, N)      # noqa: E731
    # the first point's digit is zero in the even windows and not in the odd ones, of either sign: the lanes of the wave take their
    # first row from different points
    holes = wd.from_digits([0 if w % 2 == 0 else (5 if w % 4 == 1 else -7) for w in range(62)] + [3, 0], 4)
    # every digit of the first live point negative (window 62 cannot be: it carries the value)
    negs = wd.from_digits([-8 if w % 3 else -1 for w in range(62)] + [7, 0], 4)
    assert 0 < holes < N and 0 < negs < N
    assert [d == 0 for d in wd.digits(holes, 4)[:62]] == [w % 2 == 0 for w in range(62)] and all(d < 0 for d in wd.digits(negs, 4)[:62])
    out = [("holes first", [holes] + [rs() for _ in range(n - 1)], pts),
           ("negative first", [negs] + [rs() for _ in range(n - 1)], pts),
           ("n - 1 first", [N - 1] + [rs() for _ in range(n - 1)], pts)]
    if n >= 2:
        a = rs()
        out.append(("P, -P", [a, a] + [rs() for _ in range(n - 2)], [pts[0], _neg(pts[0])] + pts[2:]))
        out.append(("P, -P, negative digits", [negs, negs] + [rs() for _ in range(n - 2)], [pts[0], _neg(pts[0])] + pts[2:]))
        out.append(("P, P", [holes, holes] + [rs() for _ in range(n - 2)], [pts[0], pts[0]] + pts[2:]))
        out.append(("identity first", [rs(), negs] + [rs() for _ in range(n - 2)], [ZERO] + pts[1:]))
    if n >= 17:
        out.append(("identities first, then P, -P, then holes", [rs(), rs(), rs(), a, a, holes] + [rs() for _ in range(n - 6)],
                    [ZERO, ZERO, ZERO, pts[3], _neg(pts[3])] + pts[5:]))
        out.append(("all but the last the identity", [rs() for _ in range(n - 1)] + [negs], [ZERO] * (n - 1) + [pts[-1]]))
    return out


@pytest.mark.parametrize("n", [1, 2, 17])
def test_window_walk_first_rows_cancellations_and_doublings(gpu, n):
    """bpgpu_msm of n points on the window-parallel route (k_verify_windows: a lane per 4-bit window, the points in turn).  The
    expected point is the oracle's MSM over the points that are not the identity."""
    assert n <= gpu.get_option("msm_wp_max")
    for name, sc, pts in _window_cases(n):
        assert len(sc) == len(pts) == n
        keep = [j for j in range(n) if pts[j] != ZERO]
        want = o.msm(o.scalars([sc[j] for j in keep]), b"".join(pts[j] for j in keep)) if keep else ZERO
        if name == "P, -P" and n == 2:
            assert want == ZERO
        assert gpu.msm(o.scalars(sc), b"".join(pts)) == want, (n, name)
