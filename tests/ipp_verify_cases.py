"""Inner-product proofs for tests/test_gpu_ipp_verify.py, made and judged by the CPU oracle alone (no GPU, no torch): importable
by the spawned worker processes that share the oracle's work (one n = 1024 proof takes it seconds to create)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

import oracle_lib as o

LABEL = b"innerproducttest"
KINDS = ("a", "b", "L", "R", "P", "Gf", "ch")       # what a tampered proof has changed


def gens(n, rot=0):
    """G, H for one proof: the oracle's chains, rotated by `rot` (per-proof generator sets differ by their rotation)"""
    Gp, Hp = o.gens("G", n), o.gens("H", n)
    r = 64 * (rot % n)
    return Gp[r:] + Gp[:r], Hp[r:] + Hp[:r]


def replay(n, L, R):
    """the verifier's transcript replay on the host (inner_product_proof.rs:269-278): challenges in creation order, final state"""
    import pymodel as pm
    t = pm.Transcript(LABEL)
    t.innerproduct_domain_sep(n)
    ch = b""
    for r in range(len(L) // 64):
        t.append_message(b"L", L[64 * r:64 * r + 64])
        t.append_message(b"R", R[64 * r:64 * r + 64])
        ch += pm.s2b(t.challenge_scalar(b"u"))
    return ch, t.state


def expect_P(n, Q, Gf, Hf, G, H, L, R, a, b, ch):
    """the reference's expect_P (:336-366) from the oracle's scalar arithmetic and MSM"""
    k = len(ch) // 32
    us, uis, s = o.verification_scalars(ch, n)
    s_rev = b"".join(s[32 * (n - 1 - i):32 * (n - i)] for i in range(n))
    zero = bytes(32)
    sc = o.sc_binop(2, a, b) + o.sc_binop(2, o.sc_binop(2, a * n, s), Gf) + o.sc_binop(2, o.sc_binop(2, b * n, s_rev), Hf)
    if k:
        sc += o.sc_binop(1, zero * k, us) + o.sc_binop(1, zero * k, uis)
    return o.msm(sc, Q + G + H + L + R)


def make(args):
    """(n, seed, rot, tamper) -> the operands of one proof as the verifier gets them (after the tampering), the oracle's verdict
    and the oracle's expect_P.  tamper: None or one of KINDS."""
    n, seed, rot, tamper = args
    G, H = gens(n, rot)
    a, b, Gf, Hf = (o.random_scalars(seed * 8 + j, n) for j in range(4))
    w = o.random_scalars(seed * 8 + 4, 1)
    Q = o.point_mul(w, o.generator())
    P = o.msm(o.sc_binop(2, a, Gf) + o.sc_binop(2, b, Hf) + o.inner_product(a, b), G + H + Q)
    L, R, ao, bo, ch = o.ipp_create(LABEL, n, Q, Gf, Hf, G, H, a, b)
    assert replay(n, L, R)[0] == ch
    one, gen = o.s2b(1), o.generator()
    if tamper == "a":
        ao = o.sc_binop(0, ao, one)
    elif tamper == "b":
        bo = o.sc_binop(0, bo, one)
    elif tamper == "L":
        L = o.point_add(L[:64], gen) + L[64:]
    elif tamper == "R":
        R = R[:-64] + o.point_add(R[-64:], gen)
    elif tamper == "P":
        P = o.point_add(P, gen)
    elif tamper == "Gf":
        Gf = o.sc_binop(0, Gf[:32], one) + Gf[32:]
    if tamper in ("L", "R"):
        ch = replay(n, L, R)[0]        # what the host's replay of the proof as received yields
    state = replay(n, L, R)[1]
    if tamper == "ch":
        ch = o.sc_binop(0, ch[:32], one) + ch[32:]
    exp = expect_P(n, Q, Gf, Hf, G, H, L, R, ao, bo, ch)
    if tamper == "ch":                 # the oracle replays its own transcript: a challenge the caller got wrong is judged by expect_P
        bit = 1 if exp == P else 0
    else:
        bit = 1 if o.ipp_verify(LABEL, n, Gf, Hf, P, Q, G, H, L, R, ao, bo) == 0 else 0
        assert bit == (1 if exp == P else 0)
    return dict(n=n, Q=Q, w=w, Gf=Gf, Hf=Hf, G=G, H=H, P=P, L=L, R=R, ab=ao + bo, ch=ch, bit=bit, expect=exp, state=state)
