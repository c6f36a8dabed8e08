"""Operands that drive the lazy F_n sums of the scalar kernels to their budgets and across their fold boundaries: Python integers only.

The discipline under test (csrc/fn_dev.cuh): a sum of Montgomery products carries its limbs but is not reduced; it is folded back with
fn_reduce every 4, 8 or 16 trips of the loop, once more before the 64-lane wave_sum, and the four waves' sums are added before the last
reduction (store_plain or fn_reduce).

What a product weighs.  mul(xR, yR) returns (T + m n) / R with T = xR * yR and 0 <= m < R = 2^261: a value in [T/R, T/R + n) that is
congruent to x y R.  T/R is below n / 500 for operands below ~n, so for non-negative operands the lazy value is the canonical
Montgomery residue x y R mod n itself, except where that residue is below T/R (then it is the residue + n).  The heaviest product is
therefore the one whose residue is n - 1: x y = -R^-1 = C.  (n - 1)(n - 1) = 1 has the residue R mod n, a 251-bit value: large, but
not the largest.  Where one operand is lazily NEGATIVE (the prover's r0 = w_O - y^i is stored as 0 - y^i R) T/R is in (-n / 500, 0]
and the same residue n - 1 comes out as n - 1 - n = -1: such terms pull the other way, which is the mixed-sign shape of the
t-coefficient sums.  tests/test_lazy_sums_cpu.py asserts these raw values on a CPU build of the headers.

No GPU needed."""
import os
import re

import mpc_dealer as md

N = md.N
R = 1 << 261
C = (-pow(R, -1, N)) % N                     # x y = C  <=>  the product's Montgomery residue is n - 1
RINV = pow(R, -1, N)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc_bulletproof_amd", "csrc")
FAMILIES = ("worst", "zero", "worst_even", "one_hot", "random")
TPB = 256                                    # threads of every block-per-sum kernel here, and of k_inner_product_partial
IP_MAX_BLOCKS = 1024                         # ip_blocks() of k_scalar.hip


def inv(x):
    return pow(x, -1, N)


def worst_pair(rnd):
    """(x, C / x): the product whose lazy value is n - 1"""
    x = rnd.randrange(1, N)
    return x, C * inv(x) % N


# ---- the kernels' own fold masks, read from the sources so that the budget assertions follow the code
SITES = {   # site -> (file, function, products added per trip at most[, the accumulator where the function folds two sums])
    "inner_product": ("k_scalar.hip", "k_inner_product_partial", 1),
    "sc_dot_batched": ("k_scalar.hip", "k_sc_dot_batched", 1),
    "prover_tcoeffs": ("k_scalar.hip", "k_prover_tcoeffs", 2),
    # a trip adds <l, r0> and one Beaver term (t2, t3: 1 + 4 products on the modifier plane) or two Beaver terms (t4: 8)
    "mpc_tcoeffs": ("k_mpc.hip", "k_mpc_tcoeffs", 8),
    "mpc_ipp_combine": ("k_mpc.hip", "k_mpc_ipp_combine", 4),
    # ---- the verifier (tests/verifier_sum_cases.py)
    "flatten_column": ("fn_dev.cuh", "flatten_column", 1),                       # a device function: one lane, serial over a column
    "vs_delta": ("k_scalar.hip", "k_verify_scalars", 1, "dpart"),
    "vs_one": ("k_scalar.hip", "k_verify_scalars", 1, "wcp"),
    "vsf_one": ("k_scalar.hip", "k_verify_scalars_fast", 1, "wcp"),
    "vsl_gh": ("k_scalar.hip", "k_vsl_gh", 1, "dpart"),
    "vsl_wc": ("k_scalar.hip", "k_vsl_wc", 1, "wcp"),
    # a trip adds one block's partial: the unreduced sum of its waves' reduced sums (VSL_TPB / 64 = 2 reduced values)
    "vsl_tail_delta": ("k_scalar.hip", "k_vsl_tail", 2, "delta"),
    "vsl_tail_wc": ("k_scalar.hip", "k_vsl_tail", 2, "wc"),
    "sc_weighted_colsum": ("k_scalar.hip", "k_sc_weighted_colsum", 1),
    "comb_colsum": ("k_pip2.hip", "comb_colsum_body", 1),
    "mix_colsum": ("k_mixed.hip", "mix_colsum_body", 1),
}
_HEAD = r"(?:__global__ void __launch_bounds__\(\w+\)|__device__ __forceinline__ (?:Fn|void)) "
# `if ((++cnt & 15) == 0) acc = fn_reduce(acc)` and k_vsl_tail's `if ((i & 7) == 7) acc = fn_reduce(acc)`
_FOLD = r"\(\+\+\w+ & (\d+)\) == 0\) (\w+) = fn_reduce\(\2\)|\(\w+ & (\d+)\) == \3\) (\w+) = fn_reduce\(\4\)"


def site_body(site):
    """the text of a site's function, from its head to the closing brace in column 0"""
    fname, func = SITES[site][:2]
    src = open(os.path.join(CSRC, fname)).read()
    body = src[re.search(_HEAD + func + r"\(", src).start():]
    return body[:body.index("\n}\n")]


def fold_trips(site):
    """the number of loop trips between two fn_reduce of a site's accumulator: mask + 1 of its `(++cnt & mask) == 0`"""
    acc = SITES[site][3] if len(SITES[site]) > 3 else None
    found = [(m.group(1) or m.group(3), m.group(2) or m.group(4)) for m in re.finditer(_FOLD, site_body(site))]
    masks = [mask for mask, name in found if acc is None or name == acc]
    assert len(masks) == 1, (site, found)
    trips = int(masks[0]) + 1
    assert trips & (trips - 1) == 0, (site, trips)
    return trips


def products_per_trip(site):
    return SITES[site][2]


def unreduced_terms(site):
    """the most lazy terms a lane's accumulator holds when it is folded: the reduced value it restarted from and a fold's products"""
    return 1 + fold_trips(site) * products_per_trip(site)


# the reduced values that meet before a last reduction: 64 lanes of a wave_sum x 4 waves; k_inner_product_finish adds 16 reduced
# partials per lane (1024 blocks / 64 lanes) before it reduces again
REDUCED_PER_BLOCK = 64 * (TPB // 64)
FINISH_PER_LANE = IP_MAX_BLOCKS // 64


# ---- lengths, each from the kernel's stride and fold
def ip_lengths():
    """bpgpu_inner_product: min(1024, ceil(n / 256)) blocks of 256, so the grid stride is 262 144 from n = 262 144 on.  262 143: the
    last length at which no lane takes a second trip; 262 145: one lane does; 524 288 + 77: every lane takes two and 77 lanes a third;
    16 trips x 262 144 = 4 194 304: every lane folds inside the loop, on its last trip; + 1000: 1000 lanes go on after the fold."""
    stride, fold = IP_MAX_BLOCKS * TPB, fold_trips("inner_product")
    return [stride - 1, stride + 1, 2 * stride + 77, fold * stride, fold * stride + 1000]


def dot_ipp_lengths():
    """k_sc_dot_batched: one block of 256 per proof over cnt = h = n / 2 elements, fold after 16 trips = 4096 elements.  IPP n = 8192:
    h = 4096, the fold on the last trip; n = 16 384: h = 8192, folds on trips 16 and 32, the first one mid-loop."""
    per_fold = TPB * fold_trips("sc_dot_batched")
    return [2 * per_fold, 4 * per_fold]


def tcoeffs_lengths():
    """k_prover_tcoeffs: a block of 256 per (proof, coefficient), fold after 8 trips = 2048 elements.  255 / 256 / 257: one trip, ragged
    and whole, and the first lane's second; 2047 / 2048 / 2049: the fold missed by one lane, met by all on the last trip, met mid-loop by
    lane 0; 2048 + 256 + 17: a whole trip and a ragged one after the fold; 4113 = 2 * 2048 + 17: two folds and a ragged trip."""
    per_fold = TPB * fold_trips("prover_tcoeffs")
    return [TPB - 1, TPB, TPB + 1, per_fold - 1, per_fold, per_fold + 1, per_fold + TPB + 17, 2 * per_fold + 17]


def mpc_tcoeffs_lengths():
    """k_mpc_tcoeffs: fold after 4 trips = 1024 elements.  1023 / 1024 / 1025 around the first fold; 1280 + 17: a whole and a ragged trip
    after it; 2048 + 256 + 3: two folds, then a whole and a ragged trip."""
    per_fold = TPB * fold_trips("mpc_tcoeffs")
    return [per_fold - 1, per_fold, per_fold + 1, per_fold + TPB + 17, 2 * per_fold + TPB + 3]


def mpc_ipp_lengths():
    """k_mpc_ipp_combine: fold after 8 trips = 2048 elements of h.  Padded n = 8192: h = 4096 is 16 trips, folds on trips 8 and 16."""
    return [4 * TPB * fold_trips("mpc_ipp_combine")]


# ---- operand families of a length: (a, b) as functions of the index through a short repeated pattern, and the sum in closed form
class Family:
    """a[i] * b[i] is C on the indices `hot` selects and 0 elsewhere; a, b repeat a short pattern of pairs, so the operands of a
    4 M-element case are bytes * count and the expected sum count * C"""

    def __init__(self, name, length, rnd, at=None, period=4):
        assert name in FAMILIES and name != "random"
        self.name, self.length, self.at = name, length, at
        self.pairs = [worst_pair(rnd) for _ in range(period)]
        assert all(x * y % N == C for x, y in self.pairs)

    def hot(self, i):
        return {"worst": True, "zero": False, "worst_even": i % 2 == 0, "one_hot": i == self.at}[self.name]

    def count(self):
        L = self.length
        return {"worst": L, "zero": 0, "worst_even": (L + 1) // 2, "one_hot": 1 if L else 0}[self.name]

    def want(self):
        return self.count() * C % N

    def a(self, i):
        return self.pairs[i % len(self.pairs)][0]

    def b(self, i):
        return self.pairs[i % len(self.pairs)][1] if self.hot(i) else 0

    def a_bytes(self):
        per = b"".join(md.le(x) for x, _ in self.pairs)
        reps, rest = divmod(self.length, len(self.pairs))
        return per * reps + per[:32 * rest]

    def b_bytes(self):
        L, P = self.length, len(self.pairs)
        if self.name == "zero":
            return bytes(32 * L)
        if self.name == "one_hot":
            out = bytearray(32 * L)
            out[32 * self.at:32 * self.at + 32] = md.le(self.b(self.at))
            return bytes(out)
        step = P if P % 2 == 0 else 2 * P                   # worst_even: a whole number of (even, odd) pairs per repeat
        per = b"".join(md.le(self.b(i)) for i in range(step))
        reps, rest = divmod(L, step)
        return per * reps + per[:32 * rest]

    def a_list(self):
        return [self.a(i) for i in range(self.length)]

    def b_list(self):
        return [self.b(i) for i in range(self.length)]


def one_hot_positions(length, stride):
    """the first index, the last one, and the first index of the second stride (where the length has one)"""
    return sorted({0, length - 1} | ({stride} if length > stride else set()))


def families(length, rnd, stride, names=("worst", "worst_even", "one_hot", "zero")):
    out = []
    for name in names:
        if name == "one_hot":
            out += [Family(name, length, rnd, at=at) for at in one_hot_positions(length, stride)]
        else:
            out.append(Family(name, length, rnd))
    return out


# ---- kernels that multiply raw planes
def tcoeffs_witness(family, n, y):
    """A witness of k_prover_polys for a circuit whose weights vanish (almost) everywhere, so that the planes are the witness:
    l1 = a_L, l2 = a_O, l3 = s_L, r0 = -y^i, r1 = y^i a_R, r3 = y^i s_R.  y is 1 or n - 1, so y^i = +-1.  The planes hold Montgomery
    forms and the kernel multiplies them unreduced: planes holding u R and v R give u v R, whose residue is n - 1 where u v = C.
    Against r0 = -y^i that needs l_k = -C y^i; with l_k so fixed, r1 = r3 = C / l_k = -y^i, i.e. a_R = s_R = n - 1.  So on the indices
    the family selects every one of the nine plane products is C; off them the l planes are 0.  (The r0 plane is lazily negative:
    those products come out as -1, not n - 1 -- see the module's text; the r1 and r3 products are n - 1.)
    -> dict of five integer lists (aL, aR, aO, sL, sR) as model_polys takes them"""
    assert y in (1, N - 1)
    lk = [(-C * (1 if i % 2 == 0 else y)) % N if family.hot(i) else 0 for i in range(n)]
    rk = [N - 1] * n
    return {"aL": list(lk), "aO": list(lk), "sL": list(lk), "aR": list(rk), "sR": list(rk)}


def plane_products(y, i):
    """the pairs (plain u, plain v) of the plane values a worst tcoeffs_witness gives at index i: (l, r0) and (l, r1) = (l, r3)"""
    yi = 1 if i % 2 == 0 else y
    l = (-C * yi) % N
    return (l, (-yi) % N), (l, yi * (N - 1) % N)


def beaver_worst(rnd, length):
    """Triples and openings of one Beaver product whose every term is worst on every plane and index: the opened d, e with
    d e = C, the triple's x = d and y = e on each plane (so d y_k = e x_k = C) and z = C (load_plain(z) is z R, residue n - 1).
    -> (d list, e list); x_k = d, y_k = e, z_k = C for k = 0, 1, 2"""
    pairs = [worst_pair(rnd) for _ in range(4)]
    d = [pairs[i % 4][0] for i in range(length)]
    e = [pairs[i % 4][1] for i in range(length)]
    return d, e


def beaver_plane_sum(length, k):
    """sum over a product's elements of z_k + d y_k + e x_k (+ d e on the modifier plane k = 2) for beaver_worst operands"""
    return length * (3 + (k == 2)) * C % N
