"""Scalars built digit by digit for the signed-window ("+K") recoding of csrc/ec29.cuh (recode_add_k / recode_digit; k_pip.hip and
pip2.cuh carry copies).  Test infrastructure, pure Python on big integers: it imports nothing from the library.
tests/test_window_digits.py checks it on the CPU, tests/test_gpu_window_digits.py drives every MSM kernel with it.

A scalar s < n becomes W = 252 // c + 1 digits d_w in [-half, half - 1], half = 2^(c-1), with sum d_w 2^(c w) = s: the digits
are the windows of s + K, K = sum_w half 2^(c w), less half each.  The range is asymmetric: magnitude `half` occurs only as the
negative extreme (a raw window plus its carry equal to half), and it selects the LAST row of a table page -- row
(g W + w) half + half - 1 -- or the last bucket of a window.  A random window is there with probability 2^-c, so at c = 16 or 20
random scalars read that row only by the tens of thousands; the battery below puts every digit worth testing into every window
on purpose.

battery(c) -> {name: scalar}.  Every entry is made from a digit vector ds; it is kept only if 0 <= from_digits(ds) < n (DROPPED
records the others: a condition, not a tuning knob), and a kept one satisfies digits(from_digits(ds), c) == ds.  With t the
largest top-window digit whose value t 2^(c (W-1)) is below n:

  w<w>:<d>      digit d alone in window w < W - 1, for d in -half, half - 1, 1, -1, -(half - 1); a negative d with +1 in window w + 1
  top:<d>       digit d alone in the top window, for d in {1, 2, t - 1, t} as far as 1 <= d <= t (a digit above t is not below n by
                the definition of t; where c divides 252 the top window starts at bit 252, t = 0 and it only ever holds a carry)
  all:<name>    a whole-scalar pattern over the windows below the top one: every digit -half, every digit half - 1, every digit
                -1, and the two alternations of -half and half - 1; the top digit is 1 where the pattern's value is negative

Where c divides 252 (4, 7, 9, 12, 14 of the widths below) a top digit 1 is worth 2^252 > n, so what needs it survives only if
the digits below take more than 2^252 - n, about 2^251, away: -half in window W - 2 does (2^252 - 2^251 = 2^251 < n), -1 and
-(half - 1) there do not, and of the patterns all -half does, all -1 and the alternation with -half in window W - 2 do not.  At
every other width nothing is dropped.
"""
N = 0x0800000000000010FFFFFFFFFFFFFFFFB781126DCAE7B2321E66A241ADC64D2F
# the Straus kernel (4), k_pip2.hip (7..12), k_pip.hip (8..16) and the fixed-base tables (4, 8, 10, 12, 14, 16, 20)
WIDTHS = (4, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 20)


def windows(c):
    return 252 // c + 1


def digits(s, c):
    """the +K model: W digits in [-half, half - 1] with sum d_w 2^(c w) = s, for 0 <= s < n"""
    W, half = windows(c), 1 << (c - 1)
    t = s + sum(half << (c * w) for w in range(W))
    assert 0 <= s < N and t >> (c * W) == 0
    return [((t >> (c * w)) & ((1 << c) - 1)) - half for w in range(W)]


def from_digits(ds, c):
    return sum(d << (c * w) for w, d in enumerate(ds))


def top_digit(c):
    """the largest digit t of the top window with t 2^(c (W-1)) < n"""
    return (N - 1) >> (c * (windows(c) - 1))


def candidates(c):
    """[(name, digit vector)] of every case of battery(c), before the value is looked at"""
    W, half = windows(c), 1 << (c - 1)
    out = []
    for w in range(W - 1):
        for d in (-half, half - 1, 1, -1, -(half - 1)):
            ds = [0] * W
            ds[w] = d
            if d < 0:
                ds[w + 1] = 1
            out.append(("w%d:%d" % (w, d), ds))
    t = top_digit(c)
    for d in sorted({1, 2, t - 1, t}):
        if 1 <= d <= t:
            out.append(("top:%d" % d, [0] * (W - 1) + [d]))
    alt = [-half if w % 2 == 0 else half - 1 for w in range(W - 1)]
    for name, low in (("-half", [-half] * (W - 1)), ("half-1", [half - 1] * (W - 1)), ("-1", [-1] * (W - 1)),
                      ("alt-half", alt), ("althalf-1", [half - 1 if d < 0 else -half for d in alt])):
        out.append(("all:" + name, low + [1 if from_digits(low, c) < 0 else 0]))
    return out


DROPPED = {}      # c -> names of the candidates whose value is not in [0, n), filled by battery(c)
_BATTERY = {}


def battery(c):
    if c not in _BATTERY:
        keep, drop = {}, []
        for name, ds in candidates(c):
            s = from_digits(ds, c)
            if 0 <= s < N:
                assert digits(s, c) == ds, (c, name)
                keep[name] = s
            else:
                drop.append(name)
        _BATTERY[c], DROPPED[c] = keep, drop
    return dict(_BATTERY[c])


def all_widths():
    """the distinct scalars of the batteries of all WIDTHS, ascending: for a test that cannot know its route's width"""
    return sorted({s for c in WIDTHS for s in battery(c).values()})
