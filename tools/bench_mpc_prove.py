#!/usr/bin/env python3
"""One party's local work of the two-party R1CS prover (include/bpgpu.h bpgpu_mpc_*) on one GPU, per call: device time (the
bpgpu_profile spans of the call's launches; bpgpu_ipp_fold and bpgpu_ipp_finish carry none and show 0) and wall time (the call as the host sees it: operand upload, launches, result download),
and the whole per-party local time of one proof with the network excluded.  Beside it: the single-party device prove of the same
circuit (the resident-witness session, host transcript) and the bytes one party sends per proof (masked values and points).
The per-party arithmetic does not depend on the values, so the operands are random field elements; the two-party proofs themselves
are checked by tests/test_gpu_mpc_prover.py.

  python tools/bench_mpc_prove.py [--quick]        circuits: 16 x 64-bit range (n = 1024) at nb = 1 and 16; the 2^14-shuffle at nb = 1"""
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mpc_dealer as md   # noqa: E402
import oracle_lib as o    # noqa: E402

pm = md.pm
N = md.N
rnd = random.Random(1)


def rand_sc(cnt):
    return b"".join(rnd.randrange(N).to_bytes(32, "little") for _ in range(cnt))


def range_circuit(nvals=16, bits=64):
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"RangeProofTest"))
    for i in range(nvals):
        v = (0x9E3779B97F4A7C15 * (i + 1)) & ((1 << bits) - 1)
        _, var = pv.commit(v, i + 1)
        pm.range_proof_gadget(pv, pm.lc_var(var), v, bits)
    return pv, False


def shuffle_circuit(k=1 << 14):
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"ShuffleProofTest"))
    xs = [(0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1) for i in range(k)]
    ys = xs[1:] + xs[:1]
    xv = [pv.commit(v, 1)[1] for v in xs]
    yv = [pv.commit(v, 1)[1] for v in ys]
    pm.shuffle_gadget(pv, xv, yv)
    pv._create_randomized_constraints()
    return pv, True


class Timer:
    def __init__(self, gpu):
        self.gpu, self.rows = gpu, []

    def __call__(self, name, fn, *a):
        self.gpu.profile_read()
        t0 = time.perf_counter()
        out = fn(*a)
        wall = (time.perf_counter() - t0) * 1e3
        prof = self.gpu.profile_read()
        # the L / R MSM span (ipp_round_msm) nests inside the round span of bpgpu_mpc_ipp_round: count it once
        dev = sum(ms for ms, _ in prof.values()) - (prof["ipp_round_msm"][0] if prof["ipp_rounds"][1] else 0.0)
        self.rows.append((name, dev, wall))
        return out


def mpc_party(gpu, gens, circ, pv, nb, n1, param, chi):
    """one party's calls for nb proofs; -> Timer rows"""
    n, m = len(pv.a_L), len(pv.v)
    n2 = n - n1
    padded = 1 << (n - 1).bit_length()
    T = Timer(gpu)
    ses, _ = T("commit phase 1", gpu.mpc_prover_commit, gens, None, nb, n1, *[rand_sc(nb * 3 * n1) for _ in range(5)], rand_sc(nb * 9))
    if n2:
        ses, _ = T("commit phase 2", gpu.mpc_prover_commit, gens, ses, nb, n2, *[rand_sc(nb * 3 * n2) for _ in range(5)], rand_sc(nb * 9))
    y, z, x, u, w = (rand_sc(nb) for _ in range(5))
    T("polys_mask", gpu.mpc_prover_polys_mask, ses, circ, nb, n, y, z, rand_sc(nb * 54 * n), chi)
    T("polys_finish", gpu.mpc_prover_polys_finish, ses, nb, m, rand_sc(nb * 12 * n), rand_sc(nb * 15))
    ipp = T("ipp_begin", gpu.mpc_prover_ipp_begin, ses, gens, padded, n1, x, u, w)
    rounds = 0
    while gpu.ipp_len(ipp) > 1:
        h = gpu.ipp_len(ipp) // 2
        T("ipp_mask (round %d)" % rounds, gpu.mpc_ipp_mask, ipp, nb, rand_sc(nb * 18 * h))
        T("ipp_round (round %d)" % rounds, gpu.mpc_ipp_round, ipp, nb, rand_sc(nb * 4 * h))
        uu = rand_sc(nb)
        T("ipp_fold (round %d)" % rounds, gpu.ipp_fold, ipp, uu, gpu.batch_inverse(uu))
        rounds += 1
    T("ipp_finish", gpu.ipp_finish, ipp, 3 * nb)
    gpu.ipp_destroy(ipp)
    gpu.prover_destroy(ses)
    return T.rows


def single_party(gpu, gens, circ, pv, nb, n1, param, chi):
    """the single-party resident-witness session of the same circuit (no two-phase split: one commit call of all n)"""
    n, m = len(pv.a_L), len(pv.v)
    padded = 1 << (n - 1).bit_length()
    T = Timer(gpu)
    ses, _ = T("commit", gpu.r1cs_prover_commit, gens, None, nb, n, rand_sc(nb * n), rand_sc(nb * n), rand_sc(nb * n), rand_sc(nb * 3),
               rand_sc(nb * n), rand_sc(nb * n))
    y, z, x, u, w = (rand_sc(nb) for _ in range(5))
    if param:
        import ctypes as C
        import mpc_bulletproof_amd as mm
        tbuf, wv = (C.c_uint8 * (32 * 6 * nb))(), (C.c_uint8 * (32 * nb * m))()
        T("session_polys_param", lambda: gpu._ck(mm.lib._lib.bpgpu_r1cs_prover_session_polys_param(gpu.ctx, ses, circ, y, z, chi, tbuf, wv)))
    else:
        T("session_polys", gpu.r1cs_prover_session_polys, ses, circ, nb, m, y, z)
    T("T commitments", gpu.msm_gens, gens, 5 * nb, 0, rand_sc(10 * nb))
    ipp = T("ipp_begin", gpu.r1cs_prover_ipp_begin, ses, gens, padded, n, x, u, None, w)
    rounds = 0
    while gpu.ipp_len(ipp) > 1:
        T("ipp_round (round %d)" % rounds, gpu.ipp_round, ipp, nb)
        uu = rand_sc(nb)
        T("ipp_fold (round %d)" % rounds, gpu.ipp_fold, ipp, uu, gpu.batch_inverse(uu))
        rounds += 1
    T("ipp_finish", gpu.ipp_finish, ipp, nb)
    gpu.ipp_destroy(ipp)
    gpu.prover_destroy(ses)
    return T.rows


def report(title, rows, nb):
    dev = sum(r[1] for r in rows)
    wall = sum(r[2] for r in rows)
    print("  %s: device %.2f ms, wall %.2f ms per call of %d proof(s) (%.2f ms wall per proof)" % (title, dev, wall, nb, wall / nb))
    return dev, wall


def main():
    import mpc_bulletproof_amd as m
    quick = "--quick" in sys.argv
    gpu = m.BpGpu(0)
    gpu.profile_enable(True)
    cases = [("16 x 64-bit range", range_circuit, (1, 16))]
    if not quick:
        cases.append(("2^14-shuffle", shuffle_circuit, (1,)))
    for title, build, nbs in cases:
        t0 = time.perf_counter()
        pv, param = build()
        n, mm_ = len(pv.a_L), len(pv.v)
        n1 = 0 if param else n
        rp, kd, ix, cf, chi0 = md.circuit_rows(pv.constraints, param=param)
        cap = 1 << (n - 1).bit_length()
        gens = gpu.gens_create(o.gens("G", cap), o.gens("H", cap), o.generator(), o.generator(), 8 if cap <= 1024 else 4)
        circ = gpu.circuit_create_param(len(pv.constraints), 1, rp, kd, ix, cf, n, mm_) if param else gpu.circuit_create(rp, kd, ix, cf, n, mm_)
        padded = cap
        k = (padded - 1).bit_length()
        print("%s: n = %d multipliers (padded %d, %d IPP rounds), q = %d, m = %d  (circuit built in %.1f s)"
              % (title, n, padded, k, len(pv.constraints), mm_, time.perf_counter() - t0))
        # what one party sends per proof: its share plane of every masked value (the modifier plane is public and alike at both
        # parties, MACs stay local until the MAC check) and its share point of every opened point
        masked_vals = 12 * n + 4 * (padded - 1)              # d, e of the 6n polynomial products and of 2 (padded_n - 1) IPP products
        points = (6 if param else 3) + 5 + 2 * k
        print("  per proof: %d triples (6n + 2 (padded_n - 1)); one party sends %d masked values x 32 B = %.2f MB and %d points x 64 B = "
              "%.1f KB" % (6 * n + 2 * (padded - 1), masked_vals, masked_vals * 32 / 1e6, points, points * 64 / 1e3))
        for nb in nbs:
            chi = chi0.to_bytes(32, "little") * nb if param else None
            mpc_party(gpu, gens, circ, pv, nb, n1, param, chi)                       # warm-up: workspaces, tables
            rows = mpc_party(gpu, gens, circ, pv, nb, n1, param, chi)
            print(" nb = %d, two-party prover, ONE party's local work:" % nb)
            for name, dev, wall in rows:
                if "round" not in name or name.endswith("(round 0)"):
                    print("    %-24s device %8.3f ms   wall %8.3f ms" % (name, dev, wall))
            rr = [r for r in rows if "(round" in r[0]]
            if rr:
                print("    %-24s device %8.3f ms   wall %8.3f ms   (all %d rounds: mask + round + fold)"
                      % ("IPP rounds total", sum(r[1] for r in rr), sum(r[2] for r in rr), k))
            report("whole local work of one party", rows, nb)
            single_party(gpu, gens, circ, pv, nb, n1, param, chi)
            rows1 = single_party(gpu, gens, circ, pv, nb, n1, param, chi)
            report("single-party device prove, same circuit", rows1, nb)
        gpu.circuit_destroy(circ)
        gpu.gens_destroy(gens)
    gpu.close()


if __name__ == "__main__":
    main()
