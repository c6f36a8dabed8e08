"""The verifier's scalar assembly (r1cs/verifier.rs:457-532) from GIVEN challenges, on Python integers: what bpgpu_r1cs_verify_batch
returns through `full` for a caller's CSR, challenges and proof scalars, and what the combined checks make of these scalars -- the
generator column sums sum_p rho_p s_{p,col} and the per-proof scalars scaled by rho_p.  The transcript plays no part: the 6 + k
challenges (y, z, u, x, w, r, u_1..u_k) are inputs, as they are for the device entry points.  tests/test_verify_scalars_model.py pins
this model to the oracle's VerifySession.msm_terms() on the golden records.

No GPU needed."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pymodel as pm          # noqa: E402

N = pm.N
KIND_L, KIND_R, KIND_O, KIND_V, KIND_ONE = 0, 1, 2, 3, 4


def coeff_ints(coeff):
    """the CSR's coefficients as integers (bytes as bpgpu_circuit_create takes them, or a list already)"""
    if isinstance(coeff, (bytes, bytearray)):
        return [int.from_bytes(coeff[i:i + 32], "little") for i in range(0, len(coeff), 32)]
    return list(coeff)


def flatten(csr, n, m, z):
    """flattened_constraints (verifier.rs:323-362) of a CSR (row_ptr, kind, idx, coeff): wL, wR, wO, wV, wc; row r weighs z^(r+1), w_V
    and w_c carry the reference's minus sign"""
    row_ptr, kind, idx, coeff = csr
    coeff = coeff_ints(coeff)
    wL, wR, wO, wV, wc = [0] * n, [0] * n, [0] * n, [0] * m, 0
    zr = 1
    for r in range(len(row_ptr) - 1):
        zr = zr * z % N
        for t in range(row_ptr[r], row_ptr[r + 1]):
            k, i, term = kind[t], idx[t], zr * coeff[t]
            if k == KIND_L:
                wL[i] += term
            elif k == KIND_R:
                wR[i] += term
            elif k == KIND_O:
                wO[i] += term
            elif k == KIND_V:
                wV[i] -= term
            else:
                assert k == KIND_ONE
                wc -= term
    red = lambda v: [x % N for x in v]                       # noqa: E731
    return red(wL), red(wR), red(wO), red(wV), wc % N


def nterms(m, k):
    return 13 + m + 2 * (1 << k) + 2 * k


def verify_scalars(csr, n, n1, m, k, challenges, proof_scalars, weights=None):
    """the 13 + m + 2 padded_n + 2k scalars of `full`, in the order of pm.Verifier.verification_msm (verifier.rs:517-532):
    A_I1 A_O1 S1 A_I2 A_O2 S2, V_0..V_{m-1}, T_1 T_3 T_4 T_5 T_6, B, B_blinding, G_0.., H_0.., L_1..L_k, R_1..R_k.
    challenges: y, z, u, x, w, r, u_1..u_k; proof_scalars: t_x, t_x_blinding, e_blinding, a, b.  weights: flatten()'s result for this z
    where the caller has it already."""
    np_ = 1 << k
    assert len(challenges) == 6 + k and len(proof_scalars) == 5 and n1 <= n <= np_
    y, z, u, x, w, r = challenges[:6]
    t_x, t_xb, e_b, a, b = proof_scalars
    wL, wR, wO, wV, wc = weights if weights is not None else flatten(csr, n, m, z)
    u_sq, u_inv_sq, s = pm.verification_scalars_from_challenges(list(challenges[6:]), np_)
    y_inv = pm.inv(y)
    pad = np_ - n
    yp, acc = [], 1
    for _ in range(np_):
        yp.append(acc)
        acc = acc * y_inv % N
    yneg_wR = [wR[i] * yp[i] % N for i in range(n)] + [0] * pad
    delta = sum(yneg_wR[i] * wL[i] for i in range(n)) % N
    u_for = [1] * n1 + [u] * (np_ - n1)
    g = [u_for[i] * (x * yneg_wR[i] - a * s[i]) % N for i in range(np_)]
    wLp, wOp = wL + [0] * pad, wO + [0] * pad
    h = [u_for[i] * (yp[i] * (x * wLp[i] + wOp[i] - b * s[np_ - 1 - i]) - 1) % N for i in range(np_)]
    xx = x * x % N
    rxx, xxx = r * xx % N, x * xx % N
    T = [r * x % N, rxx * x % N, rxx * xx % N, rxx * xxx % N, rxx * xx % N * xx % N]
    out = ([x, xx, xxx, u * x % N, u * xx % N, u * xxx % N] + [v * rxx % N for v in wV] + T
           + [(w * (t_x - a * b) + r * (xx * (wc + delta) - t_x)) % N, (-e_b - r * t_xb) % N] + g + h + u_sq + u_inv_sq)
    assert len(out) == nterms(m, k)
    return out


def affine_in_a(csr, n, n1, m, k, challenges, proof_scalars, weights=None):
    """(s0, slope): the scalars as a function of the proof scalar a are s0 + a slope exactly (only B and the g_i hold a, each to the
    first power); proof_scalars' own a is ignored"""
    ps = list(proof_scalars)
    if weights is None:
        weights = flatten(csr, n, m, challenges[1])
    s0 = verify_scalars(csr, n, n1, m, k, challenges, ps[:3] + [0] + ps[4:], weights)
    s1 = verify_scalars(csr, n, n1, m, k, challenges, ps[:3] + [1] + ps[4:], weights)
    return s0, [(q - p) % N for p, q in zip(s0, s1)]


# ---- the combined checks
def fixed_columns(m, k):
    """positions in `full` of the generator columns [B, B_blinding, G_0.., H_0..] of one proof (the rows of fixed_sc)"""
    return list(range(11 + m, 13 + m + 2 * (1 << k)))


def var_positions(m, k):
    """positions in `full` of the proof-point scalars (the rows of var_sc), in the order of the call's `points`"""
    np_ = 1 << k
    return list(range(11 + m)) + list(range(13 + m + 2 * np_, 13 + m + 2 * np_ + 2 * k))


def column_sums(fulls, rhos, m, k):
    """sum_p rho_p s_{p,col} over the generator columns of proofs of ONE shape: what k_sc_weighted_colsum / comb_colsum_body store"""
    return [sum(rho * f[c] for rho, f in zip(rhos, fulls)) % N for c in fixed_columns(m, k)]


def scaled_var(full, rho, m, k):
    """rho_p s_{p,j} over a proof's own points"""
    return [rho * full[j] % N for j in var_positions(m, k)]


def mixed_column_sums(groups):
    """the common layout [B, B_blinding, G_0..G_{nmax-1}, H_0..H_{nmax-1}] of mix_colsum_body over groups (fulls, rhos, m, k): a group
    of padded n = np adds to the first np G and H columns only"""
    nmax = max(1 << k for _, _, _, k in groups)
    out = [0] * (2 + 2 * nmax)
    for fulls, rhos, m, k in groups:
        np_ = 1 << k
        cs = column_sums(fulls, rhos, m, k)
        out[0] += cs[0]
        out[1] += cs[1]
        for i in range(np_):
            out[2 + i] += cs[2 + i]
            out[2 + nmax + i] += cs[2 + np_ + i]
    return [v % N for v in out]
