"""The arkworks in-memory forms that bpgpu_msm_ark and the bpgpu_*_ark conversions take (csrc/k_ark.hip), as Python big
integers: a Scalar is x * 2^256 mod n, a StarkPoint is Jacobian (X : Y : Z) with every coordinate c * 2^256 mod p, each value
32 little-endian bytes.  Shared by tests/test_gpu_multirank.py and tests/test_gpu_ark_edges.py."""
import oracle_lib as o


def _ark_scalar(x):
    return (x * (1 << 256) % o.N).to_bytes(32, "little")


def _ark_point(xy, z):
    """affine boundary bytes -> ark Projective bytes (Jacobian, Montgomery R = 2^256) with the given Z"""
    P = o.P
    R = 1 << 256
    if xy == bytes(64):
        return (R % P).to_bytes(32, "little") * 2 + bytes(32)          # Projective::zero() = (1 : 1 : 0)
    x, y = int.from_bytes(xy[:32], "little"), int.from_bytes(xy[32:], "little")
    X, Y = x * z * z % P, y * z * z * z % P
    return b"".join((c * R % P).to_bytes(32, "little") for c in (X, Y, z))


def _ark_point_affine(b):
    P = o.P
    Ri = pow(1 << 256, -1, P)
    X, Y, Z = (int.from_bytes(b[32 * i:32 * i + 32], "little") * Ri % P for i in range(3))
    if Z == 0:
        return bytes(64)
    zi = pow(Z, -1, P)
    return (X * zi * zi % P).to_bytes(32, "little") + (Y * zi * zi * zi % P).to_bytes(32, "little")
