"""The prover's l(x), r(x) polynomials on Python integers (prover.rs:587-619 and 659-672): the model that the GPU tests of
bpgpu_r1cs_prover_polys / _eval compare with.  No GPU needed."""
import mpc_dealer as md

N = md.N


def padded(n):
    return 1 if n == 0 else 1 << (n - 1).bit_length()


def model_polys(circ, weights, y, x, wit):
    """prover.rs:587-619 and 659-672 on integers: t_1..t_6, l_vec, r_vec with the zero / -y^i padding"""
    wL, wR, wO = weights[:3]
    n, np_ = circ.n, padded(circ.n)
    yi = pow(y, -1, N)
    l1 = [(wit["aL"][i] + pow(yi, i, N) * wR[i]) % N for i in range(n)]
    l2, l3 = wit["aO"], wit["sL"]
    r0 = [(wO[i] - pow(y, i, N)) % N for i in range(n)]
    r1 = [(pow(y, i, N) * wit["aR"][i] + wL[i]) % N for i in range(n)]
    r3 = [pow(y, i, N) * wit["sR"][i] % N for i in range(n)]
    ip = lambda a, b: sum(u * v for u, v in zip(a, b)) % N       # noqa: E731
    t = [ip(l1, r0), (ip(l1, r1) + ip(l2, r0)) % N, (ip(l2, r1) + ip(l3, r0)) % N, (ip(l1, r3) + ip(l3, r1)) % N, ip(l2, r3), ip(l3, r3)]
    lv = [x * (l1[i] + x * (l2[i] + x * l3[i])) % N for i in range(n)] + [0] * (np_ - n)
    rv = [(r0[i] + x * (r1[i] + x * x * r3[i])) % N for i in range(n)] + [(-pow(y, i, N)) % N for i in range(n, np_)]
    return t, lv, rv
