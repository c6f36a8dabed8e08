"""The lazy F_n sums of the scalar kernels (the rule of csrc/fn_dev.cuh) on a CPU build with -fsanitize=undefined, as a stand-alone
program (tests/csrc/lazysum_host_test.cpp) compared with Python integers: what the heaviest product weighs, every site's accumulate
shape -- K unreduced terms, fn_reduce, the 64-lane butterfly, the 4-wave add, the last reduction -- on the heaviest and on mixed-sign
terms, the two-level inner_product, the verifier's sites (one-wave sums, flatten_column's serial column negated and multiplied, the
h expression on two lazy columns, k_vsl_tail's partials, the weighted column sums over one and several segments, the grid-split
in-loop fold), and the two headrooms of the rule, found by bisection and held against each kernel's own fold."""
import os
import random
import re
import subprocess

import pytest

import lazy_sum_cases as lz

N, C = lz.N, lz.C
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDRS = [os.path.join(lz.CSRC, f) for f in ("fe29.cuh", "fn_dev.cuh", "kernels.h", "fe29_consts.h")]


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "csrc", "_build")
    os.makedirs(out, exist_ok=True)
    prog = os.path.join(out, "lazysum_host_test")
    src = os.path.join(HERE, "csrc", "lazysum_host_test.cpp")
    if not os.path.exists(prog) or any(os.path.getmtime(f) > os.path.getmtime(prog) for f in [src] + HDRS):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Wno-unknown-pragmas",
                               "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-o", prog, src])
    return prog


def run(exe, tmp_path, lines, check=True):
    """the program's output lines for the command lines (None where it did not end cleanly, with check=False)"""
    path = tmp_path / "cmds.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        assert not check, (r.returncode, r.stderr[-2000:])
        return None
    out = [line for line in r.stdout.split("\n") if line]
    assert len(out) == len(lines)
    return out


def limbs(text):
    """the integer a list of signed 29-bit limbs stands for"""
    return sum(int(v) << (29 * j) for j, v in enumerate(text.split(",")))


# ------------------------------------------------------------------------------------------------ the shared cases themselves
def test_families_agree_with_their_closed_forms():
    """the bytes and the closed-form sum of every structured family equal what its index-by-index definition gives"""
    rnd = random.Random(3)
    for L in (1, 2, 5, 8, 9, 23):
        fams = lz.families(L, rnd, 7)
        assert [f.at for f in fams if f.name == "one_hot"] == sorted({0, L - 1} | ({7} if L > 7 else set()))
        for fam in fams:
            a, b = fam.a_list(), fam.b_list()
            assert fam.a_bytes() == b"".join(lz.md.le(x) for x in a) and fam.b_bytes() == b"".join(lz.md.le(x) for x in b), (fam.name, L)
            assert fam.want() == sum(x * y for x, y in zip(a, b)) % N and sum(1 for y in b if y) == fam.count(), (fam.name, L)
    assert C * lz.R % N == N - 1 and lz.beaver_plane_sum(5, 2) == 20 * C % N and lz.beaver_plane_sum(5, 0) == 15 * C % N


def test_lengths_follow_the_kernels_strides_and_folds():
    assert lz.ip_lengths() == [262143, 262145, 524288 + 77, 4194304, 4194304 + 1000]
    assert lz.dot_ipp_lengths() == [8192, 16384]
    assert lz.tcoeffs_lengths() == [255, 256, 257, 2047, 2048, 2049, 2048 + 256 + 17, 4113]
    assert lz.mpc_tcoeffs_lengths() == [1023, 1024, 1025, 1280 + 17, 2048 + 256 + 3]
    assert lz.mpc_ipp_lengths() == [8192]


# ------------------------------------------------------------------------------------------------ what a product weighs
def test_the_heaviest_product_is_the_one_with_residue_n_minus_1(exe, tmp_path):
    rnd = random.Random(261)
    pairs = [lz.worst_pair(rnd) for _ in range(8)] + [((N - lz.RINV) % N, 1), (1, C), (C, 1)]
    fam = lz.Family("worst", 5, rnd)
    pairs += list(zip(fam.a_list(), fam.b_list()))
    d, e = lz.beaver_worst(rnd, 6)
    pairs += list(zip(d, e))
    out = run(exe, tmp_path, ["raw %x %x" % p for p in pairs] + ["raw %x %x" % (N - 1, N - 1), "rawload %x" % C])
    for p, line in zip(pairs, out):
        assert limbs(line) == N - 1, [hex(x) for x in p]
    # (n - 1)(n - 1) = 1: the Montgomery form of 1, far from the heaviest
    old = limbs(out[len(pairs)])
    assert old % N == lz.R % N and 0 <= old < N - 1 and old != N - 1 and old.bit_length() <= 251
    # a Beaver term's z = C is read as z R: n - 1 again
    assert limbs(out[-1]) == N - 1


@pytest.mark.parametrize("y", [1, N - 1])
def test_plane_products_of_the_worst_witness(exe, tmp_path, y):
    """the Montgomery bookkeeping of tcoeffs_witness: at every index both plane products are congruent to n - 1; the r1 / r3 one IS
    n - 1, and the one against the lazily negative r0 plane is n - 1 - n = -1 (its own heaviest value, just below zero)"""
    fam = lz.Family("worst", 9, random.Random(5))
    wit = lz.tcoeffs_witness(fam, 9, y)
    out = run(exe, tmp_path, ["plane %x %x %x %x" % (wit["aL"][i], wit["aR"][i], y, i) for i in range(9)])
    for i, line in enumerate(out):
        lr0, lr1 = [limbs(t) for t in line.split()]
        (l, r0), (l_, r1) = lz.plane_products(y, i)
        assert l == l_ == wit["aL"][i] == wit["aO"][i] == wit["sL"][i] and l * r0 % N == C and l * r1 % N == C, i
        assert lr1 == N - 1, (i, hex(lr1))
        assert lr0 == -1, (i, hex(lr0))


# ------------------------------------------------------------------------------------------------ every site's shape
def term_value(kind, a, b):
    return {0: a * b, 1: -a * b, 2: a}[kind] % N


def patterns(rnd, nt):
    """name -> pattern (a list of elements, each nt terms (kind, a, b)): the heaviest terms throughout; the heaviest on even elements
    only; mixed signs (every other term against a lazily negative factor, like <l, r0> beside <l, r1>); a Beaver element z + d y + e x
    + d e where the element has four terms; random terms"""
    worst = lambda: (0,) + lz.worst_pair(rnd)                     # noqa: E731
    out = {
        "worst": [[worst() for _ in range(nt)] for _ in range(4)],
        "worst_even": [[worst() for _ in range(nt)] if i % 2 == 0 else [(0, 0, 0)] * nt for i in range(4)],
        "mixed_sign": [[(j % 2,) + lz.worst_pair(rnd) for j in range(nt)] for _ in range(3)],
        "negative": [[(1,) + lz.worst_pair(rnd) for _ in range(nt)] for _ in range(3)],
        "random": [[(rnd.randrange(2), rnd.randrange(N), rnd.randrange(N)) for _ in range(nt)] for _ in range(7)],
    }
    if nt >= 4:
        d, e = lz.beaver_worst(rnd, 4)
        out["beaver"] = [([(2, C, 0), (0, d[i], e[i]), (0, e[i], d[i]), (0, d[i], e[i])] * nt)[:nt] for i in range(4)]
    return out


def block_lengths(fold):
    per = lz.TPB * fold
    return [0, 1, lz.TPB - 1, lz.TPB + 1, per - 1, per, per + 1, per + lz.TPB + 17, 2 * per, 2 * per + 17]


@pytest.mark.parametrize("site", ["sc_dot_batched", "prover_tcoeffs", "mpc_tcoeffs", "mpc_ipp_combine", "inner_product"])
def test_block_shape_of_each_site(exe, tmp_path, site):
    """one block of the site: its fold (read from the kernel), its products per trip, lengths around one and two folds"""
    fold, nt = lz.fold_trips(site), lz.products_per_trip(site)
    assert (fold, nt) == {"sc_dot_batched": (16, 1), "prover_tcoeffs": (8, 2), "mpc_tcoeffs": (4, 8), "mpc_ipp_combine": (8, 4),
                          "inner_product": (16, 1)}[site]
    rnd = random.Random(fold * 100 + nt)
    lines, want, what = [], [], []
    for name, pat in patterns(rnd, nt).items():
        vals = [sum(term_value(*t) for t in el) for el in pat]
        for L in block_lengths(fold):
            fin = 1 if site == "inner_product" else 0
            lines.append("block %x %x %x %x %x " % (fold, fin, L, nt, len(pat)) + " ".join("%x %x %x" % t for el in pat for t in el))
            reps, rest = divmod(L, len(pat))
            want.append((reps * sum(vals) + sum(vals[:rest])) % N)
            what.append((site, name, L))
    got = [int(x, 16) for x in run(exe, tmp_path, lines)]
    for g, w, tag in zip(got, want, what):
        assert g == w, tag


def test_two_level_inner_product(exe, tmp_path):
    """k_inner_product_partial + _finish on a grid of 4 blocks (stride 1024): the lengths of lazy_sum_cases.ip_lengths scaled to that
    stride; then _finish alone on up to 1024 heaviest partials, 16 per lane"""
    fold = lz.fold_trips("inner_product")
    grid = 4
    stride = grid * lz.TPB
    rnd = random.Random(17)
    lines, want, what = [], [], []
    pats = {"worst": [lz.worst_pair(rnd) for _ in range(4)],
            "worst_even": [lz.worst_pair(rnd), (0, 5), lz.worst_pair(rnd), (7, 0)],
            "random": [(rnd.randrange(N), rnd.randrange(N)) for _ in range(5)]}
    for name, pat in pats.items():
        vals = [a * b for a, b in pat]
        for L in (0, 1, stride - 1, stride + 1, 2 * stride + 77, fold * stride, fold * stride + 1000, 2 * fold * stride + 3):
            lines.append("ip %x %x %x %x " % (grid, fold, L, len(pat)) + " ".join("%x %x" % p for p in pat))
            reps, rest = divmod(L, len(pat))
            want.append((reps * sum(vals) + sum(vals[:rest])) % N)
            what.append(("ip", name, L))
    pat = pats["worst"]
    for nparts in (1, 63, 64, 65, 1023, lz.IP_MAX_BLOCKS):
        lines.append("finish %x %x " % (nparts, len(pat)) + " ".join("%x %x" % p for p in pat))
        want.append(nparts * C % N)
        what.append(("finish", "worst", nparts))
    got = [int(x, 16) for x in run(exe, tmp_path, lines)]
    for g, w, tag in zip(got, want, what):
        assert g == w, tag


# ------------------------------------------------------------------------------------------------ the verifier's sites
def flat_patterns(rnd):
    """name -> a list of single terms: the heaviest; the heaviest on even elements; mixed signs (every other term against a lazily
    negative factor); lazily negative throughout; random"""
    return {name: [el[0] for el in pat] for name, pat in patterns(rnd, 1).items()}


def repeat_sum(vals, count):
    reps, rest = divmod(count, len(vals))
    return reps * sum(vals) + sum(vals[:rest])


def terms_text(pat):
    return "%x " % len(pat) + " ".join("%x %x %x" % t for t in pat)


def check_lines(exe, tmp_path, lines, want, what):
    got = run(exe, tmp_path, lines)
    for g, w, tag in zip(got, want, what):
        assert [int(x, 16) for x in g.split()] == ([v % N for v in w] if isinstance(w, list) else [w % N]), tag


@pytest.mark.parametrize("site", ["vs_one", "vsf_one", "vs_delta"])
def test_one_wave_sums_of_the_verifier(exe, tmp_path, site):
    """64 lanes x fold products, then the butterfly: the `One`-column loops and the delta loop (which folds at the head of a trip)"""
    fold, stride = lz.fold_trips(site), 64
    assert fold == 16
    rnd = random.Random(site)
    per = stride * fold
    lines, want, what = [], [], []
    for name, pat in flat_patterns(rnd).items():
        vals = [term_value(*t) for t in pat]
        for L in (0, 1, 63, 65, per - 1, per, per + 1, per + stride + 17, 2 * per, 2 * per + 17, 4 * per):
            lines.append("wave %x %x %x " % (site == "vs_delta", fold, L) + terms_text(pat))
            want.append(-repeat_sum(vals, L))
            what.append((site, name, L))
    check_lines(exe, tmp_path, lines, want, what)


def test_flatten_column_shape_negated_and_multiplied(exe, tmp_path):
    """a serial run of products, folded every 16, its lazy result negated (a V column) or not, then multiplied"""
    fold = lz.fold_trips("flatten_column")
    assert fold == 16
    rnd = random.Random(16)
    lines, want, what = [], [], []
    for name, pat in flat_patterns(rnd).items():
        vals = [term_value(*t) for t in pat]
        for E in (0, 1, fold - 1, fold, fold + 1, 2 * fold - 1, 2 * fold, 2 * fold + 1, 257):
            for negate in (0, 1):
                for mult in (N - 1, 1, rnd.randrange(N)):
                    lines.append("column %x %x %x %x " % (fold, E, negate, mult) + terms_text(pat))
                    want.append((-1 if negate else 1) * repeat_sum(vals, E) * mult)
                    what.append(("column", name, E, negate))
    check_lines(exe, tmp_path, lines, want, what)


def test_h_expression_on_two_lazy_columns(exe, tmp_path):
    """h_i = y^-i (x wL + wO - b s) - 1 and delta's (wO y^-i) wL with both columns lazily as heavy as they get (15 unreduced products,
    and 16 + 15 across a fold), against heavy and random x, y^-i, b, s"""
    fold = lz.fold_trips("flatten_column")
    rnd = random.Random(17)
    lines, want, what = [], [], []
    pats = flat_patterns(rnd)
    for name, pat in pats.items():
        other = pats["worst" if name != "worst" else "mixed_sign"]
        pl, po = pat[:3], other[:3]
        vl, vo = [term_value(*t) for t in pl], [term_value(*t) for t in po]
        for E in (1, fold - 1, fold, 2 * fold - 1, 2 * fold + 1):
            for x, yi, b, sr in ((N - 1, N - 1, N - 1, N - 1), (N - 1, 1, 1, N - 1), tuple(rnd.randrange(N) for _ in range(4))):
                lines.append("hexpr %x %x %x %x %x %x " % (fold, E, x, yi, b, sr) + terms_text(pl) + " " + " ".join("%x %x %x" % t for t in po))
                wL, wO = repeat_sum(vl, E), repeat_sum(vo, E)
                want.append([yi * (x * wL + wO - b * sr) - 1, wO * yi * wL])
                what.append(("hexpr", name, E))
    check_lines(exe, tmp_path, lines, want, what)


def test_tail_of_the_grid_split_route(exe, tmp_path):
    """k_vsl_tail: up to 256 partials, each the unreduced sum of two reduced wave sums, folded every 8"""
    fold = lz.fold_trips("vsl_tail_delta")
    assert fold == lz.fold_trips("vsl_tail_wc") == 8 and lz.products_per_trip("vsl_tail_wc") == 2
    rnd = random.Random(8)
    lines, want, what = [], [], []
    for name, pat in flat_patterns(rnd).items():
        vals = [term_value(*t) for t in pat]
        for nparts in (0, 1, 7, 8, 9, 16, 17, 32, 255, 256):
            lines.append("tail %x %x 2 " % (fold, nparts) + terms_text(pat))
            want.append(-repeat_sum(vals, 2 * nparts))
            what.append(("tail", name, nparts))
    check_lines(exe, tmp_path, lines, want, what)


@pytest.mark.parametrize("site", ["sc_weighted_colsum", "comb_colsum", "mix_colsum"])
def test_weighted_column_sum_shapes(exe, tmp_path, site):
    """256 lanes x 16 trips, then four waves; mix_colsum_body's counter runs on across its segments"""
    fold = lz.fold_trips(site)
    assert fold == 16
    per = lz.TPB * fold
    rnd = random.Random(site)
    segs = [[L] for L in (0, 1, per - 1, per, per + 1, 2 * per + 17)]
    if site == "mix_colsum":
        segs += [[per // 2 + 1, per // 2 + 2], [per // 2 + 1, 0, per // 2 + 2], [per - 1, 1, 1], [3, per, 5, per + 17], [per] * 3]
    lines, want, what = [], [], []
    for name, pat in flat_patterns(rnd).items():
        vals = [term_value(*t) for t in pat]
        for lens in segs:
            lines.append("mix %x %x " % (fold, len(lens)) + " ".join("%x" % v for v in lens) + " " + terms_text(pat))
            want.append(repeat_sum(vals, sum(lens)))
            what.append((site, name, lens))
    check_lines(exe, tmp_path, lines, want, what)


@pytest.mark.parametrize("site", ["vsl_gh", "vsl_wc"])
def test_grid_split_in_loop_fold(exe, tmp_path, site):
    """128 lanes x 16 trips per block: the in-loop fold of k_vsl_gh / k_vsl_wc, which needs 256 x 128 x 16 = 2^19 elements per proof on
    the device and is covered here alone; on grids of 1, 3 and 17 blocks, then through k_vsl_tail's sum"""
    fold, tfold = lz.fold_trips(site), lz.fold_trips("vsl_tail_wc")
    assert fold == 16
    rnd = random.Random(site)
    lines, want, what = [], [], []
    for name, pat in flat_patterns(rnd).items():
        vals = [term_value(*t) for t in pat]
        for grid in (1, 3, 17):
            per = grid * 128 * fold
            for L in (per - 1, per, per + 1, 2 * per + 17):
                lines.append("split %x %x %x %x %x " % (site == "vsl_gh", fold, tfold, grid, L) + terms_text(pat))
                want.append(-repeat_sum(vals, L))
                what.append((site, name, grid, L))
    check_lines(exe, tmp_path, lines, want, what)


# ------------------------------------------------------------------------------------------------ the headrooms
def largest_ok(exe, tmp_path, cmd, cap=1 << 20):
    """the largest count up to which `cmd count x y` on a heaviest pair ends cleanly with the right sum; the first failure is looked
    for by doubling, then by bisection, and the counts on both sides of the limit are run once more"""
    x, y = lz.worst_pair(random.Random(99))

    def ok(count):
        out = run(exe, tmp_path, ["%s %x %x %x" % (cmd, count, x, y)], check=False)
        return out is not None and int(out[0], 16) == count * C % N

    hi = 1
    while ok(hi):
        hi *= 2
        assert hi <= cap
    lo = hi // 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    assert lo >= 1 and ok(lo) and not ok(lo + 1)
    return lo


@pytest.fixture(scope="module")
def headroom(exe, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("headroom")
    return largest_ok(exe, tmp, "sumraw"), largest_ok(exe, tmp, "sumred")


def test_every_kernel_stays_inside_the_measured_headroom(headroom):
    raw_limit, red_limit = headroom
    for site in lz.SITES:
        assert lz.unreduced_terms(site) <= raw_limit, (site, lz.unreduced_terms(site), raw_limit)
    assert lz.FINISH_PER_LANE <= raw_limit                       # k_inner_product_finish: reduced partials added, then fn_reduce
    assert lz.REDUCED_PER_BLOCK <= red_limit and 64 <= red_limit
    # the verifier: k_vsl_tail holds a reduced restart and a fold of partials of two reduced wave sums each; the h expression adds a
    # lazy column (at most 15 products before flatten_column's fold, or a reduced value and 15) to two products
    assert lz.unreduced_terms("vsl_tail_delta") == lz.unreduced_terms("vsl_tail_wc") == 17 <= red_limit
    assert lz.fold_trips("flatten_column") + 2 <= raw_limit
    # the limits themselves: the top limb of n is 2^19, so the 4096th heaviest term carries the int32 top limb to 2^31
    assert raw_limit == red_limit == (1 << 12) - 1


def test_the_documented_headroom_is_the_measured_one(headroom):
    """csrc/fn_dev.cuh and DESIGN.md section 3 state the two numbers this test measures"""
    raw_limit, red_limit = headroom
    rule = open(os.path.join(lz.CSRC, "fn_dev.cuh")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text, where in ((rule, "fn_dev.cuh"), (design, "DESIGN.md")):
        m = re.search(r"(\d+) unreduced products[^.]*?(\d+) reduced values", text.replace("\n//", " ").replace("\n", " "))
        assert m, where
        assert (int(m.group(1)), int(m.group(2))) == (raw_limit, red_limit), where


def test_program_refuses_a_non_canonical_value(exe, tmp_path):
    path = tmp_path / "bad.txt"
    path.write_text("raw %x 1\n" % N)
    assert subprocess.run([exe, str(path)], capture_output=True, timeout=60).returncode == 4
