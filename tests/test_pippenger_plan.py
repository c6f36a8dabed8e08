"""Which launch route the bucket-method MSM (csrc/k_pip.hip) takes for a shape, read from the library itself through the
context-free bpgpu_pippenger_plan: no device is needed.  tests/pip_shapes.py holds the shapes the GPU tests run."""
import ctypes as C

import pytest

import pip_shapes

import mpc_bulletproof_amd as m

FIELDS = m.lib.PIP_PLAN_FIELDS


def _raw_plan():
    """(nb, n) -> tuple over FIELDS, or None where the shape is refused (BPGPU_E_LEN); one output array for all calls"""
    fn, out = m.lib._lib.bpgpu_pippenger_plan, (C.c_int32 * len(FIELDS))()

    def plan(nb, n):
        rc = fn(nb, n, out)
        assert rc in (0, m.lib.E_LEN), (rc, nb, n)
        return None if rc else tuple(out)
    return plan


def test_plan_fields_follow_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bpgpu.h")).read()
    ids = {name.lower(): int(v) for name, v in re.findall(r"#define BPGPU_PIP_PLAN_([A-Z_]+) (\d+)", hdr)}
    assert ids.pop("fields") == len(FIELDS)
    assert ids == {name.lower(): i for i, name in enumerate(FIELDS)}
    out = (C.c_int32 * len(FIELDS))()
    fn = m.lib._lib.bpgpu_pippenger_plan
    assert fn(1, 1000, None) == m.lib.E_ARG and fn(0, 1000, out) == m.lib.E_ARG and fn(1, 1, out) == m.lib.E_ARG
    assert fn(1 << 20, 1 << 20, out) == m.lib.E_LEN           # what the 32-bit bucket ids and entries cannot address
    with pytest.raises(m.BpGpuError):
        m.lib.pippenger_plan(1, 0)


@pytest.mark.parametrize("key", sorted(pip_shapes.AIMED) + sorted(pip_shapes.EARLIER))
def test_shape_takes_the_route_it_is_aimed_at(key):
    pip_shapes.assert_plan(key)


def test_shapes_named_for_the_two_level_sort_that_never_took_it():
    """40 037 terms and 2 x 33 000 terms get c = 11: atomic scatter.  (The two tests that run them are named for that now.)"""
    for nb, n in ((1, 40037), (2, 33000)):
        p = m.lib.pippenger_plan(nb, n)
        assert (p["c"], p["two_level"], p["coarse_scan"]) == (11, 0, 0)
    # and the smallest shapes that do take it: c reaches 13 between 58 368 and 58 496 terms
    assert m.lib.pippenger_plan(1, 58368)["two_level"] == 0 and m.lib.pippenger_plan(1, 58496)["two_level"] == 1


def test_windows_12_and_14_are_never_chosen():
    """c in {12, 14} wins the cost formula for no n in [2, 2^21]; the windows that do win change where pip_shapes says"""
    plan = _raw_plan()
    ci = FIELDS.index("c")
    seen, changes, last = set(), [], None
    for n in range(2, (1 << 21) + 1):
        c = plan(1, n)[ci]
        if c != last:
            seen.add(c)
            changes.append((n, c))
            last = c
    assert seen == {8, 9, 10, 11, 13, 15, 16}
    assert [c for _, c in changes] == [8, 9, 10, 11, 13, 15, 16]
    for (n, _), about in zip(changes[1:], (3392, 5952, 10304, 58432, 196672, 737344)):
        assert about - 64 < n <= about, (n, about)


def test_the_tested_shapes_take_every_value_of_every_plan_field():
    """Every value that any plan field takes for any addressable (nb, n) with n <= 2^20 is taken by one of the shapes the suite
    runs on the GPU.  The sweep: every n up to 4 096, every 61st above, both sides of every power of two and of every n at which
    c changes, times instance counts on both sides of every instance threshold -- the fields are monotone step functions of n, nb
    and their products between those."""
    plan = _raw_plan()
    ns = set(range(2, 4097)) | set(range(4096, (1 << 20) + 1, 61)) | {1 << 20}
    for k in range(12, 21):
        ns |= {(1 << k) - 1, 1 << k, (1 << k) + 1} if k < 20 else {(1 << k) - 1}
    for about in (3392, 5952, 10304, 58432, 196672, 737344):
        ns |= set(range(about - 64, about + 65))
    nbs = (1, 2, 3, 4, 7, 16, 63, 64, 65, 204, 205, 1024, 1536, 1537, 2048, 2049, 4096, 65535)
    reachable = [set() for _ in FIELDS]
    for n in sorted(ns):
        for nb in nbs:
            p = plan(nb, n)
            if p is not None:
                for s, v in zip(reachable, p):
                    s.add(v)
    covered = [set() for _ in FIELDS]
    for (nb, n), _ in list(pip_shapes.AIMED.values()) + list(pip_shapes.EARLIER.values()):
        for s, v in zip(covered, plan(nb, n)):
            s.add(v)
    for name, r, c in zip(FIELDS, reachable, covered):
        assert r == c, (name, sorted(r - c), sorted(c - r))
    # what that means, spelled out: nothing a call can choose between is left to chance
    want = dict(c={8, 9, 10, 11, 13, 15, 16}, W={32, 29, 26, 23, 20, 17, 16}, two_level={0, 1}, task={16, 64}, task_search={0, 1},
                task_sort={0, 1}, scan={2, 3}, coarse_scan={0, 2, 3}, final_quad={0, 1}, chunks={1, 2, 4, 16, 64})
    assert dict(zip(FIELDS, covered)) == want
    # the new tests alone (A..I) leave only c = 9 and c = 11 (and their W, chunks = 4) to the earlier ones
    new = [set() for _ in FIELDS]
    for (nb, n), _ in pip_shapes.AIMED.values():
        for s, v in zip(new, plan(nb, n)):
            s.add(v)
    left = {name: sorted(c - a) for name, c, a in zip(FIELDS, covered, new) if c - a}
    assert left == {"c": [9, 11], "W": [23, 29], "chunks": [4]}
