"""tests/window_digits.py on the CPU: the model against itself, against the 4-bit model of degenerate_cases.py, and against the
recoding the kernels run (csrc/ec29.cuh recode_add_k / recode_digit, compiled for the host by test_device_arith_cpu.py's `h`)
for every battery scalar at every width a kernel instantiates."""
import ctypes as C

import pytest

import window_digits as wd
from test_device_arith_cpu import buf, h, le      # noqa: F401  (h: the module-scoped fixture that builds the host library)

N = wd.N


def test_widths_are_those_of_the_kernels():
    assert wd.WIDTHS == (4, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 20)
    assert [wd.windows(c) for c in wd.WIDTHS] == [64, 37, 32, 29, 26, 23, 22, 20, 19, 17, 16, 13]


@pytest.mark.parametrize("c", wd.WIDTHS)
def test_dropped_cases_are_exactly_those_not_below_n(c):
    """Nothing is dropped unless c divides 252; there a top digit 1 is worth 2^252 > n and the cases that need it are dropped unless
    the digits below take about 2^251 away (window_digits.py).  -half in window W - 2 survives at every width."""
    W, half = wd.windows(c), 1 << (c - 1)
    wd.battery(c)
    want = []
    if 252 % c == 0:
        # the alternation whose window W - 2 holds -half: 2^252 - 2^251 + (half - 1) 2^(c (W-3)) - ... > n
        alt = "all:alt-half" if (W - 2) % 2 == 0 else "all:althalf-1"
        want = ["w%d:-1" % (W - 2), "w%d:%d" % (W - 2, -(half - 1)), "all:-1", alt]
    assert wd.DROPPED[c] == want
    for name, ds in wd.candidates(c):
        s = wd.from_digits(ds, c)
        assert (name in wd.DROPPED[c]) == (not 0 <= s < N), name
        if name in wd.DROPPED[c]:
            assert s >= N and ds[W - 1] == 1 and c * (W - 1) == 252, name
    b = wd.battery(c)
    assert len(b) == len(wd.candidates(c)) - len(want)
    assert b["w%d:%d" % (W - 2, -half)] == (1 << (c * (W - 1))) - (half << (c * (W - 2)))
    t = wd.top_digit(c)
    assert (t == 0) == (252 % c == 0) and t << (c * (W - 1)) < N <= (t + 1) << (c * (W - 1))
    assert [nm for nm in b if nm.startswith("top:")] == ["top:%d" % d for d in sorted({1, 2, t - 1, t}) if 1 <= d <= t]


@pytest.mark.parametrize("c", wd.WIDTHS)
def test_battery_round_trips_and_reaches_every_extreme(c):
    W, half = wd.windows(c), 1 << (c - 1)
    seen = [set() for _ in range(W)]
    for name, s in wd.battery(c).items():
        ds = wd.digits(s, c)
        assert 0 <= s < N and len(ds) == W and all(-half <= d <= half - 1 for d in ds), name
        assert wd.from_digits(ds, c) == s, name
        for w, d in enumerate(ds):
            seen[w].add(d)
    for w in range(W - 1):      # the last row of the page, its negation's neighbour and the first row, of either sign, in every window
        want = {-half, half - 1, 1, -1, -(half - 1)}
        if 252 % c == 0 and w == W - 2:      # no scalar below n has these two there (the dropped cases)
            want -= {-1, -(half - 1)}
        assert want <= seen[w], w
    assert wd.digits(0, c) == [0] * W and wd.digits(1, c) == [1] + [0] * (W - 1)
    assert wd.from_digits(wd.digits(N - 1, c), c) == N - 1


def test_c4_model_is_the_one_of_the_degenerate_cases():
    import random

    import degenerate_cases as dc
    rnd = random.Random(4)
    for s in list(wd.battery(4).values()) + [0, 1, N - 1] + [rnd.randrange(N) for _ in range(200)]:
        assert wd.digits(s, 4) == dc.digits(s)


def test_all_widths_is_the_union():
    u = wd.all_widths()
    assert u == sorted(set(u)) and all(0 <= s < N for s in u)
    assert set(u) == {s for c in wd.WIDTHS for s in wd.battery(c).values()}
    assert 1000 <= len(u) <= sum(len(wd.battery(c)) for c in wd.WIDTHS) <= 2000


@pytest.mark.parametrize("c", wd.WIDTHS)
def test_compiled_recoding_returns_the_models_digits(h, c):      # noqa: F811
    out = (C.c_int * 80)()
    for name, s in wd.battery(c).items():
        assert h.h29_recode(c, buf(le(s)), out) == wd.windows(c)
        assert list(out)[:wd.windows(c)] == wd.digits(s, c), (c, name)
    for s in wd.all_widths():      # the other widths' scalars: ordinary digits here, the same model
        assert h.h29_recode(c, buf(le(s)), out) == wd.windows(c)
        assert list(out)[:wd.windows(c)] == wd.digits(s, c), (c, hex(s))
