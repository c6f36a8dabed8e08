#!/usr/bin/env python3
"""InnerProductProof::verify on the GPU: the one-call form against the composition of the separate exports, and resident against
explicit generators.  Writes profiles/ipp_verify.log (the source of the figures in DESIGN.md and README.md).

  (a) nb = 1, n = 2^1 .. 2^16, arbitrary generators: bpgpu_ipp_verify_batch against what the host mirror did before it --
      bpgpu_verification_scalars, the 2n products a s_i Gf_i / b s_{n-1-i} Hf_i on the host, bpgpu_msm over 2n + 2k + 1 terms.
      The host products are timed twice: as this script forms them (Python integers) and at an assumed 30 ns per modular
      multiplication (a native host's cost, the reference's ark-ff); "floor" = the two device calls alone, which no host loop
      can beat.  The new call has to hold against the floor.
  (b) nb in {256, 1024}, n in {64, 1024}: bpgpu_ipp_verify_gens (resident generator tables) against bpgpu_ipp_verify_batch over
      the same generators given as shared points.

Every timed configuration asserts its accept bits first.  Proofs are made on the GPU (bpgpu_ipp_run_fs) and P by the oracle's
MSM; (b) verifies nb copies of eight distinct proofs.  Per figure: WARM untimed calls, then REPS timed calls; median and
min..max in ms, wall clock around the synchronous call."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_lib as o   # noqa: E402
import pymodel as pm   # noqa: E402
import mpc_bulletproof_amd as m   # noqa: E402

WARM, REPS = 3, 15
NS_PER_MUL = 30e-9
LABEL = b"innerproducttest"
N = o.N
out_lines = []


def say(s=""):
    print(s)
    sys.stdout.flush()
    out_lines.append(s)


def timed(fn, reps=REPS):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return f"{t[0]:8.3f} ({t[1]:7.3f}..{t[2]:8.3f})"


def make_proofs(gpu, nb, n, seed, G, H):
    """nb proofs over shared G, H, created on the GPU -> dict of operand arrays (w: Q = w * generator)"""
    k = n.bit_length() - 1
    a, b, Gf, Hf = (o.random_scalars(seed + j, nb * n) for j in range(4))
    w = o.random_scalars(seed + 4, nb)
    B = o.generator()
    Q = b"".join(o.point_mul(w[32 * p:32 * p + 32], B) for p in range(nb))
    t = pm.Transcript(LABEL)
    t.innerproduct_domain_sep(n)
    s = gpu.ipp_begin(nb, n, Q, Gf, Hf, G, H, True, a, b)
    try:
        L, R, aa, bb, _ = gpu.ipp_run_fs(s, nb, k, t.state * nb)
    finally:
        gpu.ipp_destroy(s)
    P = ch = ab = b""
    for p in range(nb):
        sl = slice(32 * n * p, 32 * n * (p + 1))
        P += o.msm(o.sc_binop(2, a[sl], Gf[sl]) + o.sc_binop(2, b[sl], Hf[sl]) + o.inner_product(a[sl], b[sl]), G + H + Q[64 * p:64 * p + 64])
        tp = pm.Transcript(LABEL)
        tp.innerproduct_domain_sep(n)
        for r in range(k):
            tp.append_message(b"L", L[64 * (k * p + r):64 * (k * p + r + 1)])
            tp.append_message(b"R", R[64 * (k * p + r):64 * (k * p + r + 1)])
            ch += pm.s2b(tp.challenge_scalar(b"u"))
        ab += aa[32 * p:32 * p + 32] + bb[32 * p:32 * p + 32]
    return dict(Q=Q, w=w, Gf=Gf, Hf=Hf, P=P, L=L, R=R, ab=ab, ch=ch)


def main():
    gpu = m.BpGpu(0)
    say(f"# tools/bench_ipp_verify.py   warm-up {WARM}, {REPS} timed calls per figure: median (min..max) ms, wall clock of the synchronous call")
    say("## (a) one proof, arbitrary generators: bpgpu_ipp_verify_batch vs verification_scalars + host products + bpgpu_msm")
    say("# n      one call                     floor = the two device calls     + products @30 ns/mul   + products in Python   new/floor")
    base = o.gens("G", 4096) + o.gens("H", 4096)
    for lg in range(1, 17):
        n, k = 1 << lg, lg
        G = (base * ((n + 8191) // 8192))[:64 * n]
        H = ((base[64 * 7:] + base[:64 * 7]) * ((n + 8191) // 8192))[:64 * n]
        d = make_proofs(gpu, 1, n, 50 * lg, G, H)
        args = (1, n, d["Q"], d["Gf"], d["Hf"], G, H, True, d["P"], d["L"], d["R"], d["ab"], d["ch"])
        assert gpu.ipp_verify_batch(*args) == [1]
        bad = args[:11] + (d["ab"][32:] + d["ab"][:32],) + args[12:]
        assert gpu.ipp_verify_batch(*bad) == [0]
        t_new = timed(lambda: gpu.ipp_verify_batch(*args))
        # the composition, assembled as the host mirror assembled it
        a, b = o.b2s(d["ab"][:32]), o.b2s(d["ab"][32:])
        gf, hf = o.unscalars(d["Gf"]), o.unscalars(d["Hf"])
        pts = d["Q"] + G + H + d["L"] + d["R"]
        holder = {}

        def device_part():
            holder["vs"] = gpu.verification_scalars(d["ch"], n)
            return gpu.msm(holder.get("sc", bytes(32 * (2 * n + 2 * k + 1))), pts)

        def products():
            us, uis, s = (o.unscalars(x) for x in holder["vs"])
            sc = [a * b % N] + [a * s[i] % N * gf[i] % N for i in range(n)] + [b * s[n - 1 - i] % N * hf[i] % N for i in range(n)]
            sc += [(N - x) % N for x in us] + [(N - x) % N for x in uis]
            holder["sc"] = o.scalars(sc)
        device_part()
        products()
        assert device_part() == d["P"]                  # the composition accepts the same proof
        t_floor = timed(device_part)
        t_py = timed(products, reps=3 if lg > 12 else REPS)
        native = 4 * n * NS_PER_MUL * 1e3
        say(f"2^{lg:<3d} {fmt(t_new)}   {fmt(t_floor)}   {t_floor[0] + native:10.3f}            {t_floor[0] + t_py[0]:10.3f}           {t_new[0] / t_floor[0]:5.2f}")
    say()
    say("## (b) batches: resident generators (bpgpu_ipp_verify_gens, c = 8 tables) vs explicit shared generators (bpgpu_ipp_verify_batch)")
    say("# nb    n      resident                     explicit shared              resident/explicit   proofs/s resident")
    for n in (64, 1024):
        G, H, B = o.gens("G", n), o.gens("H", n), o.generator()
        g = gpu.gens_create(G, H, B, B, 8)
        d8 = make_proofs(gpu, 8, n, 4000 + n, G, H)
        per = dict(Q=64, w=32, Gf=32 * n, Hf=32 * n, P=64, L=64 * (n.bit_length() - 1), R=64 * (n.bit_length() - 1), ab=64,
                   ch=32 * (n.bit_length() - 1))
        for nb in (256, 1024):
            d = {key: b"".join(v[per[key] * (p % 8):per[key] * (p % 8 + 1)] for p in range(nb)) for key, v in d8.items()}
            # proof 3 gets a and b swapped: both outcomes in every batch
            d["ab"] = d["ab"][:64 * 3] + d["ab"][64 * 3 + 32:64 * 4] + d["ab"][64 * 3:64 * 3 + 32] + d["ab"][64 * 4:]
            want = [0 if p == 3 else 1 for p in range(nb)]
            a_res = (g, nb, n, d["w"], d["Gf"], d["Hf"], d["P"], d["L"], d["R"], d["ab"], d["ch"])
            a_exp = (nb, n, d["Q"], d["Gf"], d["Hf"], G, H, True, d["P"], d["L"], d["R"], d["ab"], d["ch"])
            assert gpu.ipp_verify_gens(*a_res) == want
            assert gpu.ipp_verify_batch(*a_exp) == want
            reps = 5 if nb * n >= 1 << 20 else REPS
            t_res = timed(lambda: gpu.ipp_verify_gens(*a_res), reps)
            t_exp = timed(lambda: gpu.ipp_verify_batch(*a_exp), reps)
            say(f"{nb:<6d} {n:<6d} {fmt(t_res)}   {fmt(t_exp)}   {t_res[0] / t_exp[0]:8.2f}            {nb / t_res[0] * 1e3:10.0f}")
        gpu.gens_destroy(g)
    gpu.close()
    path = os.path.join(ROOT, "profiles", "ipp_verify.log")
    with open(path, "w") as f:
        f.write("\n".join(out_lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
