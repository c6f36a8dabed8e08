"""Circuits, challenges and weights that drive the verifier's lazy F_n sums to their fold boundaries: Python integers only.

The verifier's operands are the caller's: bpgpu_r1cs_verify_batch takes the 6 + k challenges, bpgpu_circuit_create any CSR with
canonical coefficients, the combined calls the weights rho.  So every operand of every lazy sum of the scalar assembly can be
chosen (tests/lazy_sum_cases.py: what a product weighs, C, the families), and every scalar that comes out is compared byte for byte
with tests/verify_scalars_model.py.  The sites (lane counts and fold masks are read from the sources, lazy_sum_cases.SITES):

  flatten_column         one lane adds a column's coeff * z^(row+1), fold every 16 entries; columns >= 3n are negated; the callers
                         multiply the lazy result
  k_verify_scalars       64 lanes: the delta loop over padded_n and the `One`-column loop, fold every 16 trips of each
  k_verify_scalars_fast  (padded_n = 64, k = 6, m <= 64): the `One`-column loop; here the z powers are PLAIN, so a product's lazy value
                         is its plain residue and the heaviest coefficient is -z^-(row+1), not C z^-(row+1): both are used
  k_vsl_gh, k_vsl_wc     the same two sums split over up to 256 blocks of 128 lanes (vs_large_min = 1 sends every shape there), and
  k_vsl_tail             one lane adds the blocks' partials, fold every 8
  k_sc_weighted_colsum, comb_colsum_body, mix_colsum_body
                         256 lanes add rho_p * s_{p,col} over the proofs, fold every 16 trips; mix_colsum_body's counter runs on
                         across the segments of a mixed queue

Every challenge and weight is canonical and non-zero; coefficients are canonical (zero where a family says so).

No GPU needed."""
import random
import re

import lazy_sum_cases as lz
import mpc_dealer as md
import verify_scalars_model as vm

N, C = lz.N, lz.C
ONE = ("1",)
inv = lz.inv
VS_FAMILIES = ("worst", "worst_even", "one_hot", "zero", "random")


# ---- lane counts, from the sources
def _const(name, fname="k_scalar.hip"):
    src = open(lz.os.path.join(lz.CSRC, fname)).read()
    m = re.search(r"constexpr int [^;]*\b" + name + r" = (\d+)[,;]", src)
    assert m, name
    return int(m.group(1))


def lanes(site):
    """the lanes that share a site's sum (its loop stride)"""
    if site in ("flatten_column", "vsl_tail_delta", "vsl_tail_wc"):
        return 1
    if site in ("vs_delta", "vs_one", "vsf_one"):
        return _const("VS_TPB")
    if site in ("vsl_gh", "vsl_wc"):
        return _const("VSL_TPB")
    strides = re.findall(r"for \(size_t p = threadIdx\.x; p < [\w.]+; p \+= (\d+)\)", lz.site_body(site))
    assert len(strides) == 1, (site, strides)
    return int(strides[0])


def per_fold(site):
    return lanes(site) * lz.fold_trips(site)


def around_fold(F):
    return [F - 1, F, F + 1, 2 * F + 17]


def one_column_lengths():
    """`One` terms: 1023 / 1024 / 1025 miss the in-loop fold by one lane, meet it on every lane's last trip, pass it on lane 0;
    2065 = 2 * 1024 + 17: two folds and a ragged trip.  The fast kernel has the same stride and mask."""
    assert per_fold("vs_one") == per_fold("vsf_one")
    return around_fold(per_fold("vs_one"))


def column_entries():
    """entries of one column around flatten_column's fold: 15 (the most that stay unreduced), 16, 17, and the second fold 32, 33"""
    f = lz.fold_trips("flatten_column")
    return [f - 1, f, f + 1, 2 * f, 2 * f + 1]


def delta_sizes():
    """padded_n = 64 lanes x 16 trips puts the delta loop's fold on the last trip, twice that in mid-loop"""
    F = per_fold("vs_delta")
    return [F, 2 * F]


def split_sizes():
    """padded_n for the grid-split route: k_vsl_gh runs padded_n / 128 blocks, so 1024, 2048, 4096 hand 8, 16, 32 partials to
    k_vsl_tail: its fold on the last partial and in mid-sum"""
    t, tpb = lz.fold_trips("vsl_tail_delta"), lanes("vsl_gh")
    assert lz.fold_trips("vsl_tail_wc") == t and lanes("vsl_wc") == tpb
    return [t * tpb, 2 * t * tpb, 4 * t * tpb]


def split_parts(work):
    """verify_scalars' parts(): blocks of k_vsl_gh (work = padded_n) or k_vsl_wc (work = q)"""
    tpb, cap = lanes("vsl_gh"), _const("VSL_PARTS")
    return max(1, min(cap, (work + tpb - 1) // tpb))


def weighted_counts():
    """proofs of one combined call around the column sums' fold: 256 lanes x 16 trips"""
    F = per_fold("sc_weighted_colsum")
    assert per_fold("comb_colsum") == F == per_fold("mix_colsum")
    return around_fold(F)


def mixed_counts():
    """two segments of F / 2 + 1 and F / 2 + 2 proofs: lane 0 takes 9 trips in each, so its counter reaches 16 inside the second
    segment -- where a counter that restarted per segment would not fold at all"""
    F = per_fold("mix_colsum")
    return [F // 2 + 1, F // 2 + 2]


# ---- small helpers
def nonzero(rnd):
    return rnd.randrange(1, N)


def hot_rows(name, T, at):
    """the family's hot indices among T rows"""
    return [{"worst": True, "zero": False, "worst_even": r % 2 == 0, "one_hot": r == at}[name] for r in range(T)]


def z_inverse_powers(z, count):
    """z^-(r+1) for r < count"""
    zi, out, acc = inv(z), [], 1
    for _ in range(count):
        acc = acc * zi % N
        out.append(acc)
    return out


def challenges(rnd, k, y=None, z=None):
    ch = [nonzero(rnd) for _ in range(6 + k)]
    if y is not None:
        ch[0] = y
    if z is not None:
        ch[1] = z
    return ch


def proof_scalars(rnd):
    return [nonzero(rnd) for _ in range(5)]


def csr_of_rows(rows):
    """(row_ptr, kind, idx, coeff bytes) for bpgpu_circuit_create: mpc_dealer.circuit_rows for numeric rows, with the coefficient
    bytes joined once (a delta case has 65 536 terms)"""
    rp, kd, ix, cf = [0], [], [], []
    for row in rows:
        for var, c in row:
            assert 0 <= c < N
            kd.append(md.KIND[var[0]])
            ix.append(var[1] if len(var) > 1 else 0)
            cf.append(md.le(c))
        rp.append(len(kd))
    return rp, kd, ix, b"".join(cf)


SHAPES = {   # name -> (n, n1, m, k): the fast shape of k_verify_scalars_fast and two that are not of it
    "fast": (64, 64, 2, 6),
    "general": (13, 13, 3, 4),
    "two_phase": (5, 3, 1, 3),
}


def is_fast_shape(n, m, k):
    """verify_scalars_fast_shape for a numeric circuit"""
    return k == 6 and m <= 64


class Case:
    """one circuit and the proofs (challenges, proof scalars) to run on it; expect: closed forms of the flattened weights for the
    FIRST proofs' z (heavy_proofs of them share it)"""

    def __init__(self, name, shape, rows, proofs, heavy_proofs, expect):
        self.name = name
        self.n, self.n1, self.m, self.k = shape
        self.rows, self.proofs, self.heavy_proofs, self.expect = rows, proofs, heavy_proofs, expect
        self.q = len(rows)
        self._csr = None

    @property
    def padded_n(self):
        return 1 << self.k

    def csr(self):
        if self._csr is None:
            self._csr = csr_of_rows(self.rows)
        return self._csr

    def one_terms(self):
        return sum(1 for row in self.rows for var, _ in row if var == ONE)

    def column_lengths(self):
        out = {}
        for row in self.rows:
            for var, _ in row:
                out[var] = out.get(var, 0) + 1
        return out

    def takes_large_route(self, vs_large_min=4096):
        """vs_large() of k_scalar.hip"""
        return self.padded_n >= vs_large_min or self.m >= vs_large_min or self.q >= 4 * vs_large_min

    def model(self):
        """the scalars of every proof"""
        n, n1, m, k = self.n, self.n1, self.m, self.k
        cache = {}
        out = []
        for ch, ps in self.proofs:
            if ch[1] not in cache:
                cache[ch[1]] = vm.flatten(self.csr(), n, m, ch[1])
            out.append(vm.verify_scalars(self.csr(), n, n1, m, k, ch, ps, cache[ch[1]]))
        return out

    def check(self):
        """everything canonical and non-zero where it has to be, and the closed forms hold"""
        for ch, ps in self.proofs:
            assert len(ch) == 6 + self.k and all(0 < c < N for c in ch) and all(0 <= s < N for s in ps) and len(ps) == 5
        assert all(0 <= c < N for c in vm.coeff_ints(self.csr()[3]))
        assert self.n1 <= self.n <= self.padded_n and (self.n == 0 or self.padded_n < 2 * self.n)
        w = vm.flatten(self.csr(), self.n, self.m, self.proofs[0][0][1])
        named = dict(zip(("L", "R", "O", "V"), w[:4]))
        for key, want in self.expect.items():
            got = w[4] if key == "wc" else named[key[0]][key[1]]
            assert got == want % N, (self.name, key)
        for ch, _ in self.proofs[:self.heavy_proofs]:
            assert ch[1] == self.proofs[0][0][1] and ch[0] == self.proofs[0][0][0]


def filler_row(rnd, n, m):
    """a row of ordinary terms, so that no scalar of a case is trivially zero"""
    return [(("L", 0), nonzero(rnd)), (("R", n - 1), nonzero(rnd)), (("O", n // 2), nonzero(rnd)), (("V", m - 1), nonzero(rnd))]


# ---- the `One` column
def one_column_case(shape, T, family, rnd, at=None, plain=False):
    """T rows, each with a `One` term C z^-(row+1) on the family's rows (0 elsewhere): every product of the w_c loop is C, lazily
    n - 1 against Montgomery z powers; w_c = -count C.  plain: the coefficient is -z^-(row+1), the product n - 1 as a PLAIN value:
    the heaviest for k_verify_scalars_fast, whose z powers are plain.  Two proofs under the heavy z, one under a random z."""
    n, n1, m, k = SHAPES[shape]
    z = nonzero(rnd)
    target = N - 1 if plain else C
    if family == "random":
        coeffs = [rnd.randrange(N) for _ in range(T)]
        want = -sum(c * pow(z, r + 1, N) for r, c in enumerate(coeffs))
    else:
        hot = hot_rows(family, T, at)
        coeffs = [target * zi % N if h else 0 for zi, h in zip(z_inverse_powers(z, T), hot)]
        want = -sum(hot) * target
    rows = [[(ONE, c)] for c in coeffs]
    rows[0] = rows[0] + filler_row(rnd, n, m)
    rows[T // 2] = rows[T // 2] + filler_row(rnd, n, m)
    y = nonzero(rnd)
    proofs = [(challenges(rnd, k, y, z), proof_scalars(rnd)) for _ in range(2)] + [(challenges(rnd, k), proof_scalars(rnd))]
    name = "one %s T=%d %s%s%s" % (shape, T, family, "" if at is None else "@%d" % at, " plain" if plain else "")
    return Case(name, SHAPES[shape], rows, proofs, 2, {"wc": want})


def one_column_cases(shape, T):
    rnd = random.Random("one %s %d" % (shape, T))
    F = per_fold("vs_one")
    out = []
    for family in VS_FAMILIES:
        for at in ([0, T - 1] + ([lanes("vs_one")] if T > F else [])) if family == "one_hot" else [None]:
            out.append(one_column_case(shape, T, family, rnd, at))
    if is_fast_shape(SHAPES[shape][0], SHAPES[shape][2], SHAPES[shape][3]):
        out.append(one_column_case(shape, T, "worst", rnd, plain=True))
        out.append(one_column_case(shape, T, "worst_even", rnd, plain=True))
    return out


# ---- columns through flatten_column
def column_case(shape, E, rnd, plain=False):
    """E entries in each of L_0, R_0, O_0 (the first column), L_{n-1}, R_{n-1}, O_{n-1} (the last live one), V_0 and V_{m-1}, every
    coeff * z^(row+1) = C: each column is E C, the V columns -E C (flatten_column's negation), each lazily as heavy as E products
    get.  L and O are heavy at the same index, so x wL + wO, the sub of b s and the product by y^-i see their widest operand; so
    does delta's wL * (wR y^-i).  A last row of ordinary terms."""
    n, n1, m, k = SHAPES[shape]
    z, y = nonzero(rnd), nonzero(rnd)
    target = N - 1 if plain else C
    cols = [(kd, i) for i in (0, n - 1) for kd in "LRO"] + [("V", 0), ("V", m - 1)]
    rows = [[(var, target * zi % N) for var in cols] for zi in z_inverse_powers(z, E)]
    rows.append(filler_row(rnd, n, m) + [(ONE, nonzero(rnd))])
    last = rows[-1]
    expect = {}
    zq = pow(z, E + 1, N)
    for var in cols:
        extra = sum(c for v, c in last if v == var) * zq
        expect[var] = (E * target + extra) * (-1 if var[0] == "V" else 1)
    proofs = [(challenges(rnd, k, y, z), proof_scalars(rnd)) for _ in range(2)] + [(challenges(rnd, k), proof_scalars(rnd))]
    return Case("columns %s E=%d%s" % (shape, E, " plain" if plain else ""), SHAPES[shape], rows, proofs, 2, expect)


def column_cases(shape):
    rnd = random.Random("columns " + shape)
    out = [column_case(shape, E, rnd) for E in column_entries()]
    if shape == "fast":
        out += [column_case(shape, E, rnd, plain=True) for E in column_entries()[:3]]
    return out


# ---- delta
DELTA_L_ENTRIES = 15        # the most products flatten_column returns unreduced: the L columns are lazily 15 (n - 1)


def delta_case(padded_n, n, y_name, rnd):
    """padded_n x the delta loop: every L column holds 15 entries C z^-(row+1) (rows 0..14: w_L,i = 15 C, returned unreduced) and every
    R column one entry in row 15 with w_R,i = y^i / 15, so that w_L,i * w_R,i * y^-i = C for every i < n: delta = n C.  n < padded_n:
    the last lanes add zeros.  The coefficients hold y and z, so the heavy proofs share both; a third proof has random challenges."""
    k = padded_n.bit_length() - 1
    assert 1 << k == padded_n and padded_n // 2 < n <= padded_n
    y = {"one": 1, "minus_one": N - 1, "random": nonzero(rnd)}[y_name]
    z = nonzero(rnd)
    zi = z_inverse_powers(z, DELTA_L_ENTRIES + 1)
    rows = [[(("L", i), C * zi[r] % N) for i in range(n)] for r in range(DELTA_L_ENTRIES)]
    share, yp, last = inv(DELTA_L_ENTRIES), 1, []
    for i in range(n):
        last.append((("R", i), yp * share % N * zi[DELTA_L_ENTRIES] % N))
        yp = yp * y % N
    rows.append(last + [(("V", 0), nonzero(rnd)), (ONE, nonzero(rnd))])
    proofs = [(challenges(rnd, k, y, z), proof_scalars(rnd)) for _ in range(2)] + [(challenges(rnd, k), proof_scalars(rnd))]
    expect = {("L", 0): DELTA_L_ENTRIES * C, ("L", n - 1): DELTA_L_ENTRIES * C, ("R", 0): share,
              ("R", n - 1): pow(y, n - 1, N) * share}
    case = Case("delta np=%d n=%d y=%s" % (padded_n, n, y_name), (n, n, 1, k), rows, proofs, 2, expect)
    case.delta = n * C % N
    case.y = y
    return case


def delta_cases(padded_n):
    rnd = random.Random("delta %d" % padded_n)
    return [delta_case(padded_n, n, y_name, rnd) for n in (padded_n, padded_n - 3) for y_name in ("one", "minus_one", "random")]


def model_delta(case):
    """delta of the case's first proof from the model's weights"""
    ch = case.proofs[0][0]
    wL, wR = vm.flatten(case.csr(), case.n, case.m, ch[1])[:2]
    yi = inv(ch[0])
    return sum(wL[i] * wR[i] * pow(yi, i, N) for i in range(case.n)) % N


# ---- the weighted column sums of the combined checks
TINY = {   # name -> (n, n1, m, k)
    "np2": (2, 2, 1, 1),
    "np4": (3, 3, 1, 2),
}


class Weighted:
    """nb proofs of one tiny circuit that share their challenges and differ in the proof scalar a alone, with the weights
    rho_p = C / s_{p,col} for one generator column col: every product of that column's sum is C, the sum nb C; the other columns are
    whatever they are, and compare exactly all the same.  The scalars are affine in a: s_p = s0 + a_p slope."""

    def __init__(self, shape, nb, target, rnd):
        self.shape, self.nb, self.target = shape, nb, target
        self.n, self.n1, self.m, self.k = TINY[shape]
        n, m = self.n, self.m
        self.rows = [filler_row(rnd, n, m) + [(ONE, nonzero(rnd))], [(("L", n - 1), nonzero(rnd)), (("R", 0), nonzero(rnd))],
                     [(("O", 0), nonzero(rnd)), (("V", 0), nonzero(rnd)), (("R", n - 1), nonzero(rnd))]]
        self.csr = csr_of_rows(self.rows)
        self.ch, self.ps = challenges(rnd, self.k), proof_scalars(rnd)
        self.s0, self.slope = vm.affine_in_a(self.csr, self.n, self.n1, m, self.k, self.ch, self.ps)
        self.col = self.column(target)
        self.a, self.rho = [], []
        while len(self.a) < nb:
            a = nonzero(rnd)
            s = (self.s0[self.col] + a * self.slope[self.col]) % N
            if s:
                self.a.append(a)
                self.rho.append(C * inv(s) % N)

    def column(self, target):
        """position in `full` of the target column: "B", ("G", i) or ("H", i)"""
        np_ = 1 << self.k
        if target == "B":
            return 11 + self.m
        kind, i = target
        assert i < np_
        return 13 + self.m + i + (np_ if kind == "H" else 0)

    def full(self, p):
        return [(s + self.a[p] * d) % N for s, d in zip(self.s0, self.slope)]

    def target_sum(self):
        return sum(r * (self.s0[self.col] + a * self.slope[self.col]) for r, a in zip(self.rho, self.a)) % N

    def weighted_total(self, dl_full):
        """sum_p rho_p sum_j s_{p,j} dl_j for the dlogs dl_full of the points in the order of `full` (the same for every proof)"""
        base = sum(s * d for s, d in zip(self.s0, dl_full))
        lin = sum(s * d for s, d in zip(self.slope, dl_full))
        return (base * sum(self.rho) + lin * sum(r * a for r, a in zip(self.rho, self.a))) % N

    def column_sums(self):
        sr, sra = sum(self.rho), sum(r * a for r, a in zip(self.rho, self.a))
        return [(self.s0[c] * sr + self.slope[c] * sra) % N for c in vm.fixed_columns(self.m, self.k)]

    def check(self):
        assert all(0 < x < N for x in self.rho + self.a + self.ch) and all(0 <= x < N for x in self.ps)
        assert all(r * ((self.s0[self.col] + a * self.slope[self.col]) % N) % N == C for r, a in zip(self.rho, self.a))
        assert self.target_sum() == self.nb * C % N
        # the affine form against the model itself, on a few proofs
        for p in (0, self.nb // 2, self.nb - 1):
            ps = self.ps[:3] + [self.a[p]] + self.ps[4:]
            assert self.full(p) == vm.verify_scalars(self.csr, self.n, self.n1, self.m, self.k, self.ch, ps)
        fulls = [self.full(p) for p in (0, 1, self.nb - 1)]
        rhos = [self.rho[p] for p in (0, 1, self.nb - 1)]
        few = vm.column_sums(fulls, rhos, self.m, self.k)
        sr, sra = sum(rhos), sum(r * self.a[p] for r, p in zip(rhos, (0, 1, self.nb - 1)))
        assert few == [(self.s0[c] * sr + self.slope[c] * sra) % N for c in vm.fixed_columns(self.m, self.k)]

    # the operands of the call
    def challenge_bytes(self):
        return b"".join(md.le(c) for c in self.ch) * self.nb

    def scalar_bytes(self):
        head, tail = b"".join(md.le(s) for s in self.ps[:3]), md.le(self.ps[4])
        return b"".join(head + md.le(a) + tail for a in self.a)

    def rho_bytes(self):
        return b"".join(md.le(r) for r in self.rho)


WEIGHTED_TARGETS = ("B", ("G", 1), ("H", 1))          # B, a G column, the last H column of padded_n = 2
MIXED_TARGETS = ("B", ("G", 0), ("G", 3), ("H", 3))   # both segments add to B and G_0; G_3 and the last H column take the second alone


def weighted(nb, target):
    return Weighted("np2", nb, target, random.Random("weighted %d %s" % (nb, target)))


def mixed(target):
    """two groups of different padded_n for bpgpu_r1cs_verify_mixed_combined; a target column beyond the first group's padded_n gets
    ordinary weights there"""
    nb_a, nb_b = mixed_counts()
    rnd = random.Random("mixed %s" % (target,))
    a_target = target if target == "B" or target[1] < 2 else "B"
    return [Weighted("np2", nb_a, a_target, rnd), Weighted("np4", nb_b, target, rnd)]
