"""The arkworks in-memory forms (csrc/k_ark.hip: bpgpu_scalars_from_ark / _to_ark, bpgpu_points_from_ark / _to_ark, bpgpu_msm_ark)
at their edges: scalars next to 0, n / 2, n and the Montgomery constant, points next to the sign and x boundaries under several Z,
every spelling of the identity, non-canonical limbs, and a bad element in the last lane of a launch.  Expected values are Python
big integers; every comparison is byte equality.  Run with `-m gpu` on an MI355X."""
import random

import pytest

import codec_cases as cc
import oracle_lib as o
from ark_helpers import _ark_point, _ark_point_affine, _ark_scalar
from codec_cases import pm

pytestmark = pytest.mark.gpu
P, N = o.P, o.N
R = 1 << 256
ARK_IDENTITY = (R % P).to_bytes(32, "little") * 2 + bytes(32)        # Projective::zero() = (1 : 1 : 0), Montgomery form


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


def le(x):
    return x.to_bytes(32, "little")


def _raises_arg(fn, *args):
    import mpc_bulletproof_amd as m
    with pytest.raises(m.BpGpuError) as e:
        fn(*args)
    assert e.value.code == m.lib.E_ARG


def test_scalars_at_the_edges(gpu):
    xs = [0, 1, 2, N - 1, N - 2, (N - 1) // 2, (N + 1) // 2, 1 << 251, R % N, pow(R, -1, N)]
    assert all(0 <= x < N for x in xs)
    plain, ark = b"".join(le(x) for x in xs), b"".join(_ark_scalar(x) for x in xs)
    assert ark[32 * 9:32 * 10] == le(1) and ark[32:64] == le(R % N)
    assert gpu.scalars_to_ark(plain) == ark
    assert gpu.scalars_from_ark(ark) == plain
    # the Montgomery form of a Montgomery form, and back: x R^2 and x / R stay exact at the same edges
    assert gpu.scalars_to_ark(ark) == b"".join(le(x * R * R % N) for x in xs)
    assert gpu.scalars_from_ark(plain) == b"".join(le(x * pow(R, -1, N) % N) for x in xs)
    for bad in (N, N + 1, R - 1):
        for fn in (gpu.scalars_from_ark, gpu.scalars_to_ark):
            _raises_arg(fn, le(bad))
            _raises_arg(fn, plain + le(bad))
            _raises_arg(fn, le(bad) + plain)


@pytest.mark.parametrize("n", [127, 128, 129])
def test_one_bad_element_in_the_last_lane(gpu, n):
    rnd = random.Random(700 + n)
    xs = [rnd.randrange(N) for _ in range(n)]
    plain = b"".join(le(x) for x in xs)
    ark = b"".join(_ark_scalar(x) for x in xs)
    assert gpu.scalars_from_ark(ark) == plain and gpu.scalars_to_ark(plain) == ark
    _raises_arg(gpu.scalars_from_ark, ark[:-32] + le(N))
    _raises_arg(gpu.scalars_to_ark, plain[:-32] + le(N))
    pts = (o.gens("G", 128) + o.gens("H", 8))[:64 * n]
    ark_pts = b"".join(_ark_point(pts[64 * i:64 * i + 64], rnd.randrange(2, P)) for i in range(n))
    assert gpu.points_from_ark(ark_pts) == pts
    want = o.msm(plain, pts)
    assert _ark_point_affine(gpu.msm_ark(ark, ark_pts)) == want
    off_curve = bytearray(ark_pts)
    off_curve[-96] ^= 1                                    # X of the last point, whose Z is not 1
    _raises_arg(gpu.points_from_ark, bytes(off_curve))
    _raises_arg(gpu.msm_ark, ark, bytes(off_curve))
    _raises_arg(gpu.points_from_ark, ark_pts[:-32] + le(P))                  # Z = p
    _raises_arg(gpu.msm_ark, ark[:-32] + le(N), ark_pts)
    back = gpu.points_to_ark(pts)
    assert back == b"".join(_ark_point(pts[64 * i:64 * i + 64], 1) for i in range(n))
    bad_xy = bytearray(pts)
    bad_xy[-1] ^= 1                                        # y of the last point
    _raises_arg(gpu.points_to_ark, bytes(bad_xy))


def test_boundary_points_under_several_z(gpu):
    rnd = random.Random(77)
    b = cc.build()
    pts = list(b.sign_points) + [(x, P - y) for x, y in b.sign_points] + list(b.x_points)
    assert {x for x, _ in pts} >= {1, 2, P - 2, P - 1}
    for z in (1, 2, P - 1, rnd.randrange(3, P - 1)):
        xy = b"".join(pm.p2b(pt) for pt in pts)
        ark = b"".join(_ark_point(pm.p2b(pt), z) for pt in pts)
        assert gpu.points_from_ark(ark) == xy, z
        # the same points through the MSM: 1 * P_0 + 2 * P_1 + ...
        sc = [i + 1 for i in range(len(pts))]
        got = gpu.msm_ark(b"".join(_ark_scalar(s) for s in sc), ark)
        assert _ark_point_affine(got) == o.msm(b"".join(le(s) for s in sc), xy), z
        # off the curve with Z != 1 (and with Z = 1): refused
        for i in (0, len(pts) - 1):
            bad = bytearray(ark)
            bad[96 * i + 32] ^= 1                          # Y
            _raises_arg(gpu.points_from_ark, bytes(bad))
    assert gpu.points_to_ark(b"".join(pm.p2b(pt) for pt in pts)) == b"".join(_ark_point(pm.p2b(pt), 1) for pt in pts)


def test_identity_in_every_spelling(gpu):
    rnd = random.Random(78)
    g1 = o.gens("G", 2)
    mont = lambda c: le(c * R % P)    # noqa: E731
    spell = [ARK_IDENTITY, bytes(96), mont(rnd.randrange(P)) + mont(rnd.randrange(P)) + bytes(32), le(P - 1) + le(P - 1) + bytes(32),
             mont(5) + bytes(64)]
    assert gpu.points_from_ark(b"".join(spell)) == bytes(64 * len(spell))
    for s in spell:
        assert gpu.points_from_ark(s) == bytes(64)
        # as an operand of a sum it adds nothing
        got = gpu.msm_ark(_ark_scalar(3) + _ark_scalar(5), s + _ark_point(g1[:64], 7))
        assert _ark_point_affine(got) == o.point_mul(o.s2b(5), g1[:64])
    # non-canonical limbs are refused even where Z = 0 would make the point the identity
    _raises_arg(gpu.points_from_ark, le(P) + le(1) + bytes(32))
    _raises_arg(gpu.points_from_ark, le(1) + le(P) + bytes(32))
    _raises_arg(gpu.points_from_ark, _ark_point(g1[:64], 1)[:64] + le(P))
    _raises_arg(gpu.points_from_ark, ARK_IDENTITY + le(R - 1) + le(1) + bytes(32))
    _raises_arg(gpu.msm_ark, _ark_scalar(1), le(P) + le(1) + bytes(32))
    # the identity goes out as (1 : 1 : 0), byte for byte
    assert gpu.points_to_ark(bytes(64)) == ARK_IDENTITY
    assert gpu.points_to_ark(g1[:64] + bytes(64) + g1[64:]) == _ark_point(g1[:64], 1) + ARK_IDENTITY + _ark_point(g1[64:], 1)
    assert gpu.msm_ark(b"", b"") == ARK_IDENTITY                                               # n = 0
    neg = g1[:32] + le(P - int.from_bytes(g1[32:64], "little"))
    assert gpu.msm_ark(_ark_scalar(1) * 2, _ark_point(g1[:64], 9) + _ark_point(neg, 4)) == ARK_IDENTITY      # P + (-P)
    assert gpu.msm_ark(_ark_scalar(6) + _ark_scalar(N - 6), _ark_point(g1[:64], 1) * 2) == ARK_IDENTITY      # 6 P + (n - 6) P
    for n in (1, 3, 40):
        pts = b"".join(_ark_point(o.gens("H", n)[64 * i:64 * i + 64], 2 + i) for i in range(n))
        assert gpu.msm_ark(bytes(32 * n), pts) == ARK_IDENTITY, n                               # all-zero scalars
    assert gpu.msm_ark(_ark_scalar(9) * 2, ARK_IDENTITY + bytes(96)) == ARK_IDENTITY           # identity operands only
