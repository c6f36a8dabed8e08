"""tests/verifier_sum_cases.py checked on the CPU: the lengths follow the kernels' own strides and fold masks (changing a mask in
the sources fails here), every circuit, challenge and weight is canonical, every crafted product is C, the closed forms agree with
tests/verify_scalars_model.py, and every case reaches the trip count it is there for.  No GPU needed."""
import pytest

import lazy_sum_cases as lz
import verifier_sum_cases as vc
import verify_scalars_model as vm

N, C = vc.N, vc.C


def test_lengths_follow_the_kernels_strides_and_folds():
    assert {s: (vc.lanes(s), lz.fold_trips(s)) for s in lz.SITES if s not in ("inner_product", "sc_dot_batched", "prover_tcoeffs",
                                                                                "mpc_tcoeffs", "mpc_ipp_combine")} == {
        "flatten_column": (1, 16), "vs_delta": (64, 16), "vs_one": (64, 16), "vsf_one": (64, 16), "vsl_gh": (128, 16), "vsl_wc": (128, 16),
        "vsl_tail_delta": (1, 8), "vsl_tail_wc": (1, 8), "sc_weighted_colsum": (256, 16), "comb_colsum": (256, 16), "mix_colsum": (256, 16)}
    assert vc.one_column_lengths() == [1023, 1024, 1025, 2065]
    assert vc.column_entries() == [15, 16, 17, 32, 33]
    assert vc.delta_sizes() == [1024, 2048]
    assert vc.split_sizes() == [1024, 2048, 4096]
    assert vc.weighted_counts() == [4095, 4096, 4097, 8209]
    assert vc.mixed_counts() == [2049, 2050]
    assert vc.DELTA_L_ENTRIES == lz.fold_trips("flatten_column") - 1


def trips(count, stride, lane=0):
    """loop trips of one lane of a strided loop over `count` elements"""
    return max(0, (count - lane + stride - 1) // stride)


@pytest.mark.parametrize("shape", ["fast", "two_phase"])
def test_one_column_cases(shape):
    stride, fold = vc.lanes("vs_one"), lz.fold_trips("vs_one")
    n, n1, m, k = vc.SHAPES[shape]
    assert vc.is_fast_shape(n, m, k) == (shape == "fast") and (shape == "fast") == (n == 1 << k == 64)
    seen = []
    for T in vc.one_column_lengths():
        cases = vc.one_column_cases(shape, T)
        assert sum(1 for c in cases if "one_hot" in c.name) == (3 if T > stride * fold else 2)
        assert sum(1 for c in cases if "plain" in c.name) == (2 if shape == "fast" else 0)
        for c in cases:
            c.check()
            assert c.one_terms() == T and c.q == T and not c.takes_large_route() and c.takes_large_route(1)
            ch = c.proofs[0][0]
            if "worst" in c.name.split()[3]:
                hot = T if "worst_even" not in c.name else (T + 1) // 2
                target = N - 1 if "plain" in c.name else C
                assert c.expect["wc"] % N == -hot * target % N
                # every hot product is the target itself
                coeff = vm.coeff_ints(c.csr()[3])
                ones = [t for t, kd in enumerate(c.csr()[1]) if kd == vm.KIND_ONE]
                assert all(coeff[t] * pow(ch[1], r + 1, N) % N in (target, 0) for r, t in enumerate(ones))
        seen.append((trips(T, stride), trips(T, stride, stride - 1)))
        # the grid-split route's partial count for this row count
    # lane 0 / the last lane: 16 | 15, 16 | 16, 17 | 16, 33 | 32 trips: the fold missed by one lane, on the last trip, passed, passed twice
    assert seen == [(16, 15), (16, 16), (17, 16), (33, 32)]
    assert [vc.split_parts(T) for T in vc.one_column_lengths()] == [8, 8, 9, 17]
    t = lz.fold_trips("vsl_tail_wc")
    assert vc.split_parts(vc.one_column_lengths()[1]) == t and vc.split_parts(vc.one_column_lengths()[3]) == 2 * t + 1


@pytest.mark.parametrize("shape", ["fast", "general"])
def test_column_cases(shape):
    n, n1, m, k = vc.SHAPES[shape]
    cases = vc.column_cases(shape)
    assert [c.name.split()[2] for c in cases[:5]] == ["E=15", "E=16", "E=17", "E=32", "E=33"]
    for c, E in zip(cases, vc.column_entries() + vc.column_entries()[:3]):
        c.check()
        target = N - 1 if "plain" in c.name else C
        lens = c.column_lengths()
        heavy = [(kd, i) for i in (0, n - 1) for kd in "LRO"] + [("V", 0), ("V", m - 1)]
        extra = {var: sum(1 for v, _ in c.rows[-1] if v == var) for var in heavy}
        assert all(lens[var] == E + extra[var] for var in heavy), c.name
        # the columns no ordinary term touches are exactly +-E C: first column R, O; last live column L, O; V_0
        for var in heavy:
            if not extra[var]:
                assert c.expect[var] % N == (-1 if var[0] == "V" else 1) * E * target % N
        assert sum(1 for var in heavy if not extra[var]) >= 5
        assert not c.takes_large_route() and c.takes_large_route(1)


@pytest.mark.parametrize("padded_n", [1024, 2048, 4096])
def test_delta_cases(padded_n):
    stride, fold = vc.lanes("vs_delta"), lz.fold_trips("vs_delta")
    cases = vc.delta_cases(padded_n)
    assert [(c.n, c.y) for c in cases[:3]] == [(padded_n, 1), (padded_n, N - 1), (padded_n, cases[2].y)] and cases[2].y not in (1, N - 1)
    assert [c.n for c in cases[3:]] == [padded_n - 3] * 3
    for c in cases:
        c.check()
        assert c.padded_n == padded_n and c.q == vc.DELTA_L_ENTRIES + 1 and c.q < 4 * 4096
        assert c.takes_large_route() == (padded_n >= 4096)
        ch = c.proofs[0][0]
        wL, wR = vm.flatten(c.csr(), c.n, c.m, ch[1])[:2]
        yi = vc.inv(ch[0])
        assert all(wL[i] * wR[i] * pow(yi, i, N) % N == C for i in (0, 1, 2, c.n // 2, c.n - 2, c.n - 1))
        assert vc.model_delta(c) == c.delta == c.n * C % N
        assert all(c.column_lengths()[("L", i)] == vc.DELTA_L_ENTRIES for i in (0, c.n - 1))
    # every lane takes padded_n / 64 trips: 16 (the fold on the last trip), 32, 64
    assert trips(padded_n, stride) == trips(padded_n, stride, stride - 1) == padded_n // stride and padded_n // stride % fold == 0
    assert vc.split_parts(padded_n) == padded_n // 128


def test_weighted_cases():
    stride, fold = vc.lanes("sc_weighted_colsum"), lz.fold_trips("sc_weighted_colsum")
    assert [(trips(nb, stride), trips(nb, stride, stride - 1)) for nb in vc.weighted_counts()] == [(16, 15), (16, 16), (17, 16), (33, 32)]
    for nb in vc.weighted_counts():
        for target in vc.WEIGHTED_TARGETS:
            w = vc.weighted(nb, target)
            w.check()
            assert w.nb == nb and (w.n, w.m, w.k) == (2, 1, 1)
            cols = w.column_sums()
            assert cols[vm.fixed_columns(w.m, w.k).index(w.col)] == nb * C % N
    assert vm.fixed_columns(1, 1)[-1] == vc.weighted(4, ("H", 1)).col       # the last H column


def test_mixed_cases():
    stride, fold = vc.lanes("mix_colsum"), lz.fold_trips("mix_colsum")
    nb_a, nb_b = vc.mixed_counts()
    # lane 0: 9 trips in the first segment, the fold (trip 16) on its 7th trip of the second, 18 in all; no segment folds on its own
    assert trips(nb_a, stride) == 9 and trips(nb_b, stride) == 9 and trips(nb_a, stride) < fold < trips(nb_a, stride) + trips(nb_b, stride)
    for target in vc.MIXED_TARGETS:
        a, b = vc.mixed(target)
        a.check()
        b.check()
        assert (a.nb, b.nb) == (nb_a, nb_b) and (1 << a.k, 1 << b.k) == (2, 4)
        mixed = vm.mixed_column_sums([([g.full(p) for p in range(g.nb)], g.rho, g.m, g.k) for g in (a, b)])
        ca, cb = a.column_sums(), b.column_sums()
        want = [ca[0] + cb[0], ca[1] + cb[1]] + [cb[2 + i] + (ca[2 + i] if i < 2 else 0) for i in range(4)] \
            + [cb[6 + i] + (ca[4 + i] if i < 2 else 0) for i in range(4)]
        assert mixed == [v % N for v in want]
        j = 0 if target == "B" else 2 + target[1] + (4 if target[0] == "H" else 0)
        both = target == "B" or target[1] < 2
        assert mixed[j] == ((nb_a + nb_b) if both else nb_b) * C % N
