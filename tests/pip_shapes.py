"""The shapes at which the suite runs the bucket-method MSM (csrc/k_pip.hip), each with the launch route it is aimed at, as
bpgpu_pippenger_plan reports it (include/bpgpu.h BPGPU_PIP_PLAN_*; mpc_bulletproof_amd.lib.pippenger_plan).  One table for
tests/test_pippenger_plan.py, which checks it on the CPU and shows that the shapes together take every route a call can take,
and for the GPU tests of tests/test_gpu_parity.py, each of which asserts its row before it compares a point: a threshold that
moves makes the test fail instead of leaving its route unnoticed.

Where the plan fields come from (pippenger_plan in k_pip.hip), with W = 252 / c + 1 windows of half = 2^(c-1) buckets:
  c            argmin over 8..16 of W (n + 3 half); the winners change at about 3 392, 5 952, 10 304, 58 432, 196 672 and 737 344 terms
  two_level    c >= 12 and n >= 2^15
  task         64 when n / half >= 12 and nb W half >= 2^18, otherwise 16
  task_search  (n >> (252 - c (W - 1))) / task > 64
  task_sort    nb n W >= 2^18
  scan         3 when the nb W half bucket counts fill more than 4 096 tiles of 2 048, otherwise 2
  coarse_scan  the same for the nb W 256 ceil(n / 8 192) coarse histogram entries of the two-level sort; 0 without it
  final_quad   nb > 1 536
  chunks       min(64, max(1, half / 256))
"""

# (nb, n) -> the plan fields the shape is aimed at.  A..I: the new GPU tests (test_msm_pippenger_route_*).
AIMED = {
    "A": ((1, 6000), dict(c=10, W=26, two_level=0, task=16, task_search=1, task_sort=0, scan=2, coarse_scan=0, final_quad=0, chunks=2)),
    "B": ((64, 1536), dict(c=8, W=32, two_level=0, task=64, task_search=0, task_sort=1, scan=2, coarse_scan=0, final_quad=0, chunks=1)),
    "C": ((1, 58437), dict(c=13, W=20, two_level=1, task=16, task_search=1, task_sort=1, scan=2, coarse_scan=2, final_quad=0, chunks=16)),
    "D": ((4, 58437), dict(c=13, W=20, two_level=1, task=64, task_search=0, task_sort=1, scan=2, coarse_scan=2, final_quad=0, chunks=16)),
    "E": ((1, 196700), dict(c=15, W=17, two_level=1, task=64, task_search=0, task_sort=1, scan=2, coarse_scan=2, final_quad=0, chunks=64)),
    "F": ((1, 737400), dict(c=16, W=16, two_level=1, task=64, task_search=0, task_sort=1, scan=2, coarse_scan=2, final_quad=0, chunks=64)),
    "G1536": ((1536, 16), dict(c=8, W=32, two_level=0, task=16, task_search=0, task_sort=1, scan=2, coarse_scan=0, final_quad=0, chunks=1)),
    "G1537": ((1537, 16), dict(c=8, W=32, two_level=0, task=16, task_search=0, task_sort=1, scan=2, coarse_scan=0, final_quad=1, chunks=1)),
    "G2049": ((2049, 16), dict(c=8, W=32, two_level=0, task=16, task_search=0, task_sort=1, scan=3, coarse_scan=0, final_quad=1, chunks=1)),
    "H2": ((1, 2), dict(c=8, W=32, two_level=0, task=16, task_search=0, task_sort=0, scan=2, coarse_scan=0, final_quad=0, chunks=1)),
    "H3": ((1, 3), dict(c=8, two_level=0, task=16, task_sort=0)),
    "H17": ((1, 17), dict(c=8, two_level=0, task=16, task_sort=0)),
    "H255": ((1, 255), dict(c=8, two_level=0, task=16, task_sort=0)),
    # the scan of the coarse histograms in three launches: 205 x 20 segments x 256 bins x 8 tiles = 8 396 800 entries, the fewest
    # terms at which a two-level call has more than 4 096 x 2 048 of them (c = 13 is the smallest two-level window, 8 tiles its
    # smallest tile count, and the last tile is the raggedest one there: 1 093 of 8 192 keys)
    "I": ((205, 58437), dict(c=13, W=20, two_level=1, task=64, task_search=0, task_sort=1, scan=3, coarse_scan=3, final_quad=0, chunks=16)),
}
# the bucket-method shapes the suite had before: test_msm_pippenger_sizes (512, 5 000 and 98 347 terms), test_msm_batch_pippenger
# (2 x 700), and the two tests that were named for the two-level sort although 40 037 and 2 x 33 000 terms take the atomic scatter
EARLIER = {
    "sizes512": ((1, 512), dict(c=8, two_level=0, task=16, task_search=0, task_sort=0, chunks=1)),
    "sizes5000": ((1, 5000), dict(c=9, W=29, two_level=0, task=16, task_search=1, task_sort=0, chunks=1)),
    "sizes98347": ((1, 98347), dict(c=13, W=20, two_level=1, task=16, task_search=1, task_sort=1, coarse_scan=2, chunks=16)),
    "batch700": ((2, 700), dict(c=8, two_level=0, task=16)),
    "skewed40037": ((1, 40037), dict(c=11, W=23, two_level=0, task=16, task_search=0, task_sort=1, scan=2, coarse_scan=0, final_quad=0, chunks=4)),
    "batch33000": ((2, 33000), dict(c=11, W=23, two_level=0, task=16, task_search=0, task_sort=1, scan=2, coarse_scan=0, final_quad=0, chunks=4)),
}


def assert_plan(key):
    """the (nb, n) of a row, after asserting that the library routes it as the row says"""
    from mpc_bulletproof_amd.lib import pippenger_plan
    (nb, n), want = (AIMED.get(key) or EARLIER[key])
    plan = pippenger_plan(nb, n)
    got = {k: plan[k] for k in want}
    assert got == want, (key, nb, n, plan)
    return nb, n
