"""Inputs and expected outputs of bpgpu_r1cs_commit_values / bpgpu_mpc_commit_values from the Python model (oracle/pymodel.py):
V = pt_add(pt_mul(v, B), pt_mul(v_blinding, B_blinding)), its boundary and compressed bytes, and the hash chain from the state the
host holds when it would call Prover::new -- r1cs_domain_sep, then append_point("V", V_j) in order.  No GPU needed;
tests/test_commit_values_abi.py checks these expectations against the model prover's own commit()."""
import random

import circuit_gen as cg
import mpc_dealer as md
import oracle_lib as o
import prove_fs2_cases as pc2
import prove_fs_cases as pc
import window_digits as wd

pm = md.pm
N = pm.N
mont = md.mont

# (nb, m) and the launch route of the point path at c = 8 (nb m < 64: a block per MSM; < 1024: 32 lanes per MSM; else 16), and
# the blocks of the chain launch (a lane per prover, 64 per block)
SHAPES = [(1, 1), (1, 0), (3, 2), (2, 17), (9, 7), (8, 8), (5, 13), (70, 1), (2, 515)]
# the three point routes of the edge batches: commitments per batch, as (nb, m)
EDGE_SHAPES = [(2, 5), (7, 10), (2, 515)]


def base_G():
    return pm.G


def base_H0():
    """the first H generator: a second Pedersen base that is not the curve generator"""
    return pm.b2p(o.gens("H", 1))


def label(p):
    return b"CommitValues #%d" % p


def init_states(nb):
    """the chain state of prover p when the host would call Prover::new: a fresh transcript under the prover's label"""
    return [pm.Transcript(label(p)).state for p in range(nb)]


def values(seed, nb, m):
    """(v, v_blinding) as nb x m integers"""
    rnd = random.Random(seed)
    return ([[rnd.randrange(N) for _ in range(m)] for _ in range(nb)], [[rnd.randrange(N) for _ in range(m)] for _ in range(nb)])


def ark(rows):
    """nb x m integers -> the call's operand bytes (ark-ff Montgomery form)"""
    return b"".join(mont(x) for row in rows for x in row)


_mul = {}


def mul(k, base):
    """pm.pt_mul, computed once per (scalar, base): the model takes milliseconds per multiplication, and the same values meet
    several pairs of bases and several tests"""
    key = (k % N, base)
    if key not in _mul:
        _mul[key] = pm.pt_mul(k, base)
    return _mul[key]


def commit(v, vb, B, Bb):
    """the model's commitment (PedersenGens.commit over the bases B, B_blinding)"""
    return pm.pt_add(mul(v, B), mul(vb, Bb))


def expect(v, vb, B, Bb, states):
    """-> dict(points: nb x m model points, V, V_compressed, states_out: the bytes the call is expected to return)"""
    pts, out = [], b""
    for p, st in enumerate(states):
        tr = pm.Transcript(b"")
        tr.state = st
        tr.r1cs_domain_sep()
        row = [commit(a, b, B, Bb) for a, b in zip(v[p], vb[p])]
        for pt in row:
            tr.append_point(b"V", pt)
        pts.append(row)
        out += tr.state
    flat = [pt for row in pts for pt in row]
    return dict(points=pts, V=b"".join(map(pm.p2b, flat)), V_compressed=b"".join(map(pm.point_compress, flat)), states_out=out)


# ---- edge pairs over equal bases: sums that vanish, sums that double, digits at the ends of their range
X = 0x0123456789ABCDEF0FEDCBA9876543210123456789ABCDEF0FEDCBA987654321 % N
IDENTITY_PAIRS = [(0, 0), (X, N - X)]
LISTED_PAIRS = [(0, 0), (0, X), (X, 0), (1, 1), (5, 5), (X, X), (X, N - X), (N - 1, N - 1), (N - 1, 1), (1 << 251, 1 << 251)]


def window_pairs(c):
    """pairs of scalars whose every window digit below the top one is an extreme of the signed recoding at width c (-2^(c-1), or
    2^(c-1) - 1, the largest positive digit): equal scalars -- over equal bases both terms read the SAME table rows -- and the
    two extremes against each other"""
    b = wd.battery(c)
    ext = [b[k] for k in ("all:-half", "all:half-1", "all:alt-half", "all:althalf-1") if k in b]
    assert len(ext) >= 2, c
    return [(s, s) for s in ext] + [(ext[0], ext[1]), (ext[-1], ext[-2])]


def edge_batches(c, nb, m):
    """The batches of one route: nb x m commitments each, holding every listed pair and every window pair of width c, padded with
    the random pairs of values(1000 nb + m, nb, m) -- what the tests of this shape commit to anyway, so the model multiplies them
    once.  One batch when it has room for all the pairs, else the listed pairs in the first and the window pairs in the second.
    -> [(v, v_blinding)] as nb x m integers"""
    tot = nb * m
    rv, rb = values(1000 * nb + m, nb, m)
    pad = [(a, b) for xs, ys in zip(rv, rb) for a, b in zip(xs, ys)]
    groups = [LISTED_PAIRS + window_pairs(c)] if tot >= len(LISTED_PAIRS) + len(window_pairs(c)) else [LISTED_PAIRS, window_pairs(c)]
    out = []
    for pairs in groups:
        assert len(pairs) <= tot
        pairs = list(pairs) + pad[len(pairs):]
        out.append(([[pairs[p * m + j][0] for j in range(m)] for p in range(nb)], [[pairs[p * m + j][1] for j in range(m)] for p in range(nb)]))
    return out


# ---- the provers that follow the commit call: model proofs of generated circuits (tests/prove_fs_cases.py, prove_fs2_cases.py)
class ModelGens:
    """the model's BulletproofGens interface over the oracle's generator chain"""

    def __init__(self, cap):
        self.gens_capacity = cap
        self._g = [pm.b2p(b) for b in md.cut(o.gens("G", cap), 64)]
        self._h = [pm.b2p(b) for b in md.cut(o.gens("H", cap), 64)]

    def G(self, n, share=0):
        return self._g[:n]

    def H(self, n, share=0):
        return self._h[:n]


# (n, m, q, nb, profile) of the one-phase chain, and the two-phase shape (prove_fs2_cases.SHAPES[3]) with its provers
CHAIN_SHAPES = [(3, 2, 7, 3, "sparse"), (5, 5, 12, 3, "dups+holes"), (2, 0, 3, 2, "sparse")]
CHAIN2_SHAPE, CHAIN2_NB = pc2.SHAPES[3], 2
_proofs = {}


def chain_case(shape):
    """the circuit of a one-phase shape and the model's records of its nb provers, explicit blinding vectors (computed once)"""
    if shape not in _proofs:
        n, m, q, nb, profile = shape
        circ = cg.Circuit(500 + 10 * n + m, n, 0, m, q, 0, profile)
        mg = ModelGens(16)
        _proofs[shape] = (circ, [pc.model_proof(circ, mg, p, False, 500 + n) for p in range(nb)])
    return _proofs[shape]


def chain2_case():
    """the same for the two-phase shape"""
    if CHAIN2_SHAPE not in _proofs:
        circ = pc2.circuit(CHAIN2_SHAPE)
        mg = ModelGens(16)
        _proofs[CHAIN2_SHAPE] = (circ, [pc2.model_proof(circ, mg, p, (False, False), 700 + CHAIN2_SHAPE[0]) for p in range(CHAIN2_NB)])
    return _proofs[CHAIN2_SHAPE]
