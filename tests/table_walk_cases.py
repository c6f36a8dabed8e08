"""Cases for tests/test_gpu_table_walk_prefetch.py: shapes at which a table walk that fetches a row one addition ahead of its use can
go wrong -- a row paired with the wrong digit, a fetch past the end of a run of generators, an identity row added.  Test
infrastructure, pure Python: it imports nothing from the library.

Generators of a verification MSM are numbered as the fixed-base kernels number them: 0 = B, 1 = B_blinding, 2 + i = G_i,
2 + n + i = H_i.  In the oracle's list of MSM terms (oracle/bpo_r1cs.c) they are the terms 11 + m ... 12 + m + 2 n, in the same order;
the proof points before them are the first 11 + m operands of bpgpu_r1cs_verify_batch, the L_j and R_j follow the generators.
"""
import random

import window_digits as wd

ZERO = bytes(64)       # the identity, as the ABI and the oracle encode it

# ---------------------------------------------------------------- identity generators of the 8-bit gadget (18 generators)
# Runs of 3 generators are [0..2] [3..5] ... [15..17]; runs of 5 are [0..4] [5..9] [10..14] and the short [15..17].
IDENTITY_SETS = {
    "b_blinding": (1,),
    "chunk_edges": (3, 5, 9, 15),     # first and last of a run of 3; first (5, 15) and last (9) of a run of 5
    "last_of_all": (17,),
    "consecutive": (7, 8),
    "combined": (1, 5, 9, 12, 13, 17),
}
CHUNK_LENGTHS = (1, 3, 5, 9, 18)       # 18: the one run the option allows (no partial sums: the lanes-per-proof walk)
BATCHES = (64, 65, 130)                # a full wave; one live lane in the last wave; a ragged last wave


def gens_with_identities(G, H, B, Bb, which):
    """the four operands of bpgpu_gens_create with the numbered generators replaced by the identity"""
    n = len(G) // 64
    flat = [B, Bb] + [G[64 * i:64 * i + 64] for i in range(n)] + [H[64 * i:64 * i + 64] for i in range(n)]
    for i in which:
        flat[i] = ZERO
    return b"".join(flat[2:2 + n]), b"".join(flat[2 + n:]), flat[0], flat[1]


def drop_terms(scalars, points, drop):
    """the oracle's MSM terms without the terms `drop` (identity points: they contribute nothing)"""
    n = len(scalars) // 32
    keep = [t for t in range(n) if t not in drop]
    return b"".join(scalars[32 * t:32 * t + 32] for t in keep), b"".join(points[64 * t:64 * t + 64] for t in keep)


# ---------------------------------------------------------------- scalars with zero digits at chosen windows
def with_zero_windows(c, zero, seed):
    """a scalar below n whose signed digits (window_digits.digits) are zero exactly at the windows `zero` and nowhere else"""
    W, half = wd.windows(c), 1 << (c - 1)
    rnd = random.Random(seed)
    top = wd.top_digit(c)
    assert top >= 2 or (W - 1) in zero, "the top window of this width holds only a carry"
    ds = []
    for w in range(W):
        if w in zero:
            ds.append(0)
        elif w == W - 1:
            ds.append(rnd.randrange(1, top))
        else:
            ds.append(rnd.choice([rnd.randrange(-half, 0), rnd.randrange(1, half)]))
    hi = max(w for w in range(W) if ds[w] != 0)
    ds[hi] = abs(ds[hi])               # the value is positive
    if ds[hi] == half:
        ds[hi] = half - 1
    s = wd.from_digits(ds, c)
    assert 0 <= s < wd.N and wd.digits(s, c) == ds, (c, zero)
    return s


# ---------------------------------------------------------------- identity points among the 87 proof points of 64 one-bit values
NVAR_MULTI = 87                        # 11 + m + 2 k with m = 64, k = 6: two chunks of the window kernel, 64 + 23 points
POINT_PATTERNS = {                     # operands replaced by the identity (3, 4, 5 are the identity in every one-phase proof)
    "as_is": (),
    "first": (0,),
    "last_of_chunk": (63,),
    "first_of_chunk_and_last_of_all": (64, 86),
    "across_the_chunk_boundary": (62, 63, 64, 65),
    "all_but_one_in_chunk_two": tuple(j for j in range(NVAR_MULTI) if j != 70),
    "all_but_one_in_chunk_one": tuple(j for j in range(NVAR_MULTI) if j != 2),
    "all": tuple(range(NVAR_MULTI)),
}


def msm_patterns(n):
    """(name, identity points, zero scalars) of an n-term MSM through the window-parallel launches: groups of 16 points from 33
    terms on, one group below"""
    return [("as_is", (), ()), ("first", (0,), ()), ("last", (n - 1,), ()),
            ("group_edges_and_two_in_a_row", (15, 16, 20, 21), ()),
            ("all_but_one", tuple(j for j in range(n) if j != 17), ()),
            ("zero_scalar", (), (5,)), ("one_scalar_left", (), tuple(j for j in range(n) if j != 30)),
            ("all", tuple(range(n)), ())]
