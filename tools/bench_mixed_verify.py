#!/usr/bin/env python3
"""Mixed-queue verification (bpgpu_r1cs_verify_mixed_screened_dev) against what a host does without it.  One process, one context,
device-resident operands; A and B interleaved, medians of --reps calls each.  The proofs are a REPLAYED pool: --pool (2 048) distinct
proofs per circuit made by the CPU oracle (tests/oracle_lib.py) in --jobs processes before the GPU is opened and kept in --pool-cache,
repeated to the queue length, each copy with its own random weight.  The generator tables of M1 / M2 use --window-bits (20, as
bench.py); M3's 4 098 generators use window 8 on both sides (a window-16 / 20 table of that many would not fit the GPU).
  M1  262 144 valid 64-bit range proofs as ONE group: mixed_screened_dev vs bpgpu_r1cs_verify_screened_dev
  M2  64-bit range 50 %, 16-bit range 25 %, 4 x 16-bit range 15 %, example gadget 10 % at 4 096 / 16 384 / 65 536 proofs:
      one mixed_screened_dev vs one bpgpu_r1cs_verify_screened_dev per circuit in sequence on the same context
  M3  one 2^10-shuffle (parametric) + 4 096 64-bit range proofs: one mixed call vs bpgpu_r1cs_verify_batch_param for the shuffle
      plus a screened call for the ranges
  W   the M2 mix as WIRE bytes (R1CSProof::to_bytes, compressed commitments, transcript states; sizes of --m2-sizes), three ways on
      the same queue: (1) one bpgpu_r1cs_verify_mixed_wire_screened_dev; (2) one bpgpu_r1cs_verify_batch_wire_dev per circuit in
      sequence, all a host can do without (1); (3) bpgpu_r1cs_verify_mixed_screened_dev on operands decoded and challenged
      beforehand, the floor.  Every accept bit is asserted.
Prints one JSON line per measurement and appends it to --log (profiles/mixed_verify.log).  --pools-only makes the oracle pools (no
GPU needed) and exits.
Usage: bench_mixed_verify.py [--only M1,M2,M3,W] [--pool 2048] [--reps 7] [--m2-sizes 4096,16384,65536] [--window-bits 20]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import bp_helpers as bh  # noqa: E402
import oracle_lib as o  # noqa: E402
import mpc_bulletproof_amd as m  # noqa: E402


def lib_hash():
    import hashlib
    with open(m.lib.SO_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


# name -> (kind, param, label, generator capacity the proofs are made with)
SPECS = {"range64": (o.K_RANGE, 64, b"RangeProofTest", 64), "range16": (o.K_RANGE, 16, b"RangeProofTest", 64),
         "multi4x16": (o.K_RANGE_MULTI, 16 | (4 << 16), b"RangeProofTest", 64), "example": (o.K_EXAMPLE, 0, b"R1CSExampleGadget", 64),
         "shuffle1024": (o.K_SHUFFLE, 1024, b"ShuffleProofTest", 2048)}


def _values(name, rnd):
    """-> (prover values, verifier values) of one proof"""
    if name == "range64":
        return [rnd.getrandbits(64)], []
    if name == "range16":
        return [rnd.getrandbits(16)], []
    if name == "multi4x16":
        return [rnd.getrandbits(16) for _ in range(4)], []
    if name == "example":         # (a1 + a2)(b1 + b2) = c1 + c2, the public c2 = 9 fixed: one circuit
        a, b, c, d = (rnd.randrange(2, 50) for _ in range(4))
        return [a, b, c, d, (a + b) * (c + d) - 9, 9], [9]
    x = [rnd.getrandbits(40) for _ in range(1024)]
    return x + rnd.sample(x, len(x)), []


def _make_proof(job):
    """one pool proof by the CPU oracle (a worker process) -> operands (+ dims and the CSR of the circuit)"""
    name, i = job
    kind, param, label, cap = SPECS[name]
    vals, vvals = _values(name, random.Random(sum(name.encode()) * 1000003 + i))
    rc, proof, com = o.r1cs_prove(kind, param, label, vals, 4000 + i, cap)
    assert rc == 0
    s = o.VerifySession(kind, param, label, vvals, com, proof, cap)
    assert s.rc == 0
    k, pts, sc = bh.verify_inputs(proof, com)
    chi = b""
    if kind == o.K_SHUFFLE:           # the gadget challenge z: the oracle's rows carry -z as the `One` coefficients
        _, kd, _, cf = s.csr()
        ones = {cf[32 * t:32 * t + 32] for t in range(len(kd)) if kd[t] == 4}
        chi = o.s2b((o.N - o.b2s(ones.pop())) % o.N)
    out = dict(rec=(pts, sc, s.challenges(), chi), dims=(s.n1, s.k, s.m, s.n1 + s.n2, s.q), csr=s.csr() if i == 0 else None)
    s.close()
    return out


def pool_records(name, npool, cache_dir, jobs):
    """npool distinct proofs of one circuit, made once by the oracle in `jobs` processes and kept in cache_dir (before any GPU use)"""
    import multiprocessing as mp
    import pickle
    path = os.path.join(cache_dir, f"{name}_{npool}.pkl") if cache_dir else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    with mp.get_context("fork").Pool(jobs) as pool:
        made = pool.map(_make_proof, [(name, i) for i in range(npool)], chunksize=8)
    out = dict(recs=[x["rec"] for x in made], dims=made[0]["dims"], csr=made[0]["csr"])
    if path:
        os.makedirs(cache_dir, exist_ok=True)
        with open(path + ".tmp", "wb") as f:
            pickle.dump(out, f)
        os.replace(path + ".tmp", path)
    return out


def _wire_of(job):
    """operands of one pool proof -> (R1CSProof::to_bytes, compressed commitments) through the Python model (a worker process)"""
    import pymodel as pm
    pts, sc, k, m_ = job
    pt = [pm.b2p(pts[64 * i:64 * i + 64]) for i in range(11 + m_ + 2 * k)]
    p = dict(zip(("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2"), pt[:6]))
    p.update(zip(("T_1", "T_3", "T_4", "T_5", "T_6"), pt[6 + m_:11 + m_]))
    p.update(zip(("t_x", "t_x_blinding", "e_blinding", "a", "b"), (pm.b2s(sc[32 * i:32 * i + 32]) for i in range(5))))
    p["L_vec"], p["R_vec"] = pt[11 + m_:11 + m_ + k], pt[11 + m_ + k:]
    return pm.r1cs_proof_to_bytes(p), b"".join(pm.point_compress(v) for v in pt[6:6 + m_])


def pool_wire(name, data, npool, cache_dir, jobs):
    """the wire form of a pool's proofs, made once beside the pool (before any GPU use)"""
    import multiprocessing as mp
    import pickle
    path = os.path.join(cache_dir, f"{name}_{npool}_wire.pkl") if cache_dir else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            return pickle.load(f)
    k, m_ = data["dims"][1], data["dims"][2]
    with mp.get_context("fork").Pool(jobs) as pool:
        out = pool.map(_wire_of, [(r[0], r[1], k, m_) for r in data["recs"]], chunksize=32)
    if path:
        with open(path + ".tmp", "wb") as f:
            pickle.dump(out, f)
        os.replace(path + ".tmp", path)
    return out


class Pool:
    """pool proofs of one circuit, operands in the layouts of bpgpu_r1cs_verify_batch, and the circuit on the device"""

    def __init__(self, gpu, name, data):
        self.recs = data["recs"]
        self.n1, self.k, self.m, self.n, self.q = data["dims"]
        csr = data["csr"]
        self.param = SPECS[name][0] == o.K_SHUFFLE
        if self.param:
            rp, kd, ix, cf = csr
            rows0, rows1 = [[] for _ in range(self.q)], [[] for _ in range(self.q)]
            for r in range(self.q):
                for t in range(rp[r], rp[r + 1]):
                    (rows1[r].append((4, 0, (o.N - 1).to_bytes(32, "little"))) if kd[t] == 4 else
                     rows0[r].append((kd[t], ix[t], cf[32 * t:32 * t + 32])))
            prp, pkd, pix, pcf = [0], [], [], []
            for row in rows0 + rows1:
                for a, b, c in row:
                    pkd.append(a)
                    pix.append(b)
                    pcf.append(c)
                prp.append(len(pkd))
            self.circ = gpu.circuit_create_param(self.q, 1, prp, pkd, pix, b"".join(pcf), self.n, self.m)
        else:
            self.circ = gpu.circuit_create(*csr, self.n, self.m)

    def device(self, gpu, nb, rnd):
        """nb replayed proofs resident in HBM -> group dict of device pointers (+ ok), list of allocations"""
        reps = [self.recs[i % len(self.recs)] for i in range(nb)]
        g = dict(circuit=self.circ, nb=nb, n1=self.n1, k=self.k)
        allocs = []
        for f, j in (("points", 0), ("scalars", 1), ("challenges", 2)):
            g[f] = gpu.to_device(b"".join(r[j] for r in reps))
            allocs.append(g[f])
        g["gadget_challenges"] = None
        if self.param:
            g["gadget_challenges"] = gpu.to_device(b"".join(r[3] for r in reps))
            allocs.append(g["gadget_challenges"])
        g["rho"] = gpu.to_device(b"".join(o.s2b(rnd.randrange(1, o.N)) for _ in range(nb)))
        g["ok"] = gpu.malloc(4 * nb)
        allocs += [g["rho"], g["ok"]]
        return g, allocs

    def device_wire(self, gpu, name, nb, rho, wires):
        """the same nb replayed proofs as wire bytes -> bpgpu_wire_group dict of device pointers (the weights are shared with `device`)"""
        import pymodel as pm
        reps = [wires[i % len(wires)] for i in range(nb)]
        g = dict(circuit=self.circ, nb=nb, n1=self.n1, proof_len=len(reps[0][0]), gadget_label=None, rho=rho)
        g["proofs"] = gpu.to_device(b"".join(r[0] for r in reps))
        g["commitments"] = gpu.to_device(b"".join(r[1] for r in reps))
        g["init_states"] = gpu.to_device(pm.Transcript(SPECS[name][2]).state * nb)
        g["ok"] = gpu.malloc(4 * nb)
        return g, [g["proofs"], g["commitments"], g["init_states"], g["ok"]]


def timed(gpu, fn):
    gpu.sync()
    t = time.perf_counter()
    r = fn()
    gpu.sync()
    return time.perf_counter() - t, r


def ab(gpu, a, b, reps):
    ta, tb = [], []
    for _ in range(2):                                   # untimed lead-in of both
        timed(gpu, a)
        timed(gpu, b)
    for i in range(reps):
        for which, fn, dst in ((0, a, ta), (1, b, tb)) if i % 2 == 0 else ((1, b, tb), (0, a, ta)):
            dt, r = timed(gpu, fn)
            assert r == 0, ("fallback batches on valid proofs", which, r)
            dst.append(dt)
    return statistics.median(ta), statistics.median(tb)


def abc(gpu, fns, reps):
    """medians of `reps` interleaved calls of each of fns (rotating the order); every call must report no fallback"""
    ts = [[] for _ in fns]
    for _ in range(2):
        for fn in fns:
            timed(gpu, fn)
    for i in range(reps):
        for j in range(len(fns)):
            w = (i + j) % len(fns)
            dt, r = timed(gpu, fns[w])
            assert not r, ("fallback batches on valid proofs", w, r)
            ts[w].append(dt)
    return [statistics.median(t) for t in ts]


def all_ok(gpu, groups):
    for g in groups:
        raw = gpu.download(g["ok"], 4 * g["nb"])
        assert raw == b"\x01\x00\x00\x00" * g["nb"], "a valid proof was rejected"


def screened_one(gpu, gens, g):
    return gpu.r1cs_verify_screened_dev(gens, g["circuit"], g["nb"], g["n1"], g["k"], g["points"], g["scalars"], g["challenges"],
                                        g["rho"], g["ok"])


LOG = None


def emit(**kw):
    kw["lib"] = LIB
    line = json.dumps(kw)
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="M1,M2,M3")
    ap.add_argument("--pool", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--m2-sizes", default="4096,16384,65536")
    ap.add_argument("--window-bits", type=int, default=20, help="table window of the generators of M1 / M2 (bench.py's default)")
    ap.add_argument("--pool-cache", default=os.path.join(ROOT, "tools", "_wl", "mixed_pools"),
                    help="directory of the oracle proof pools (made on first use)")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1), help="processes that make the pools")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "mixed_verify.log"), help="file the JSON lines are appended to ('' = none)")
    ap.add_argument("--pools-only", action="store_true", help="make the oracle pools of --only (no GPU needed) and exit")
    args = ap.parse_args()
    global LOG
    LOG = args.log or None
    which = set(args.only.split(","))
    t0 = time.perf_counter()
    mix_names = ["range16", "multi4x16", "example"]
    names = ["range64"] + (mix_names if which & {"M2", "W"} else []) + (["shuffle1024"] if "M3" in which else [])
    data = {n: pool_records(n, args.pool if n != "shuffle1024" else 1, args.pool_cache, args.jobs) for n in names}
    wires = {n: pool_wire(n, data[n], args.pool, args.pool_cache, args.jobs) for n in ["range64"] + mix_names} if "W" in which else {}
    if args.pools_only:
        return
    print(f"# pools ready in {time.perf_counter() - t0:.1f} s ({args.pool} distinct oracle proofs per circuit, replayed; one 2^10-shuffle)",
          file=sys.stderr, flush=True)
    gpu = m.BpGpu(0)
    rnd = random.Random(1)
    allocs = []
    cap = 64
    # the generator tables of bench.py (--window-bits, default 20: 130 generators x 13 windows x 2^19 entries = 57 GB at capacity 64)
    gens = gpu.gens_create(o.gens("G", cap), o.gens("H", cap), o.generator(), o.generator(), args.window_bits)
    p64 = Pool(gpu, "range64", data["range64"])
    if which & {"M2", "W"}:
        p16, pm4, pex = (Pool(gpu, n, data[n]) for n in mix_names)
    if "M1" in which:
        nb = 262144
        g, al = p64.device(gpu, nb, rnd)
        allocs += al
        ta, tb = ab(gpu, lambda: gpu.r1cs_verify_mixed_screened_dev(gens, [g]), lambda: screened_one(gpu, gens, g), args.reps)
        all_ok(gpu, [g])
        emit(metric="M1", proofs=nb, mixed_ms=ta * 1e3, one_circuit_ms=tb * 1e3, mixed_per_s=nb / ta, one_circuit_per_s=nb / tb,
             ratio_mixed_over_one=ta / tb, reps=args.reps, window_bits=args.window_bits, pool=args.pool)
    if "M2" in which:
        for tot in [int(x) for x in args.m2_sizes.split(",")]:
            parts = [(p64, tot // 2), (p16, tot // 4), (pm4, tot * 15 // 100), (pex, tot - tot // 2 - tot // 4 - tot * 15 // 100)]
            groups = []
            for pool, nb in parts:
                g, al = pool.device(gpu, nb, rnd)
                allocs += al
                groups.append(g)

            def per_circuit():
                return sum(screened_one(gpu, gens, g) for g in groups)
            ta, tb = ab(gpu, lambda: gpu.r1cs_verify_mixed_screened_dev(gens, groups), per_circuit, args.reps)
            all_ok(gpu, groups)
            emit(metric="M2", proofs=tot, mixed_ms=ta * 1e3, per_circuit_ms=tb * 1e3, speedup=tb / ta, reps=args.reps, window_bits=args.window_bits, pool=args.pool)
    if "W" in which:
        for tot in [int(x) for x in args.m2_sizes.split(",")]:
            parts = [("range64", p64, tot // 2), ("range16", p16, tot // 4), ("multi4x16", pm4, tot * 15 // 100),
                     ("example", pex, tot - tot // 2 - tot // 4 - tot * 15 // 100)]
            groups, wgroups = [], []
            for name, pool, nb in parts:
                g, al = pool.device(gpu, nb, rnd)
                wg, wal = pool.device_wire(gpu, name, nb, g["rho"], wires[name])
                allocs += al + wal
                groups.append(g)
                wgroups.append(wg)

            def per_circuit_wire():
                for wg in wgroups:
                    gpu.r1cs_verify_batch_wire_dev(gens, wg["circuit"], wg["nb"], wg["n1"], wg["proof_len"], wg["proofs"], wg["commitments"],
                                                   wg["init_states"], wg["ok"])
                return 0
            for wg in wgroups:                                # every leg's accept bits, each from a cleared array
                gpu.upload(wg["ok"], bytes(4 * wg["nb"]))
            assert gpu.r1cs_verify_mixed_wire_screened_dev(gens, wgroups) == 0
            gpu.sync()
            all_ok(gpu, wgroups)
            for wg in wgroups:
                gpu.upload(wg["ok"], bytes(4 * wg["nb"]))
            per_circuit_wire()
            gpu.sync()
            all_ok(gpu, wgroups)
            t1, t2, t3 = abc(gpu, [lambda: gpu.r1cs_verify_mixed_wire_screened_dev(gens, wgroups), per_circuit_wire,
                                   lambda: gpu.r1cs_verify_mixed_screened_dev(gens, groups)], args.reps)
            all_ok(gpu, wgroups)
            all_ok(gpu, groups)
            emit(metric="W", proofs=tot, mixed_wire_ms=t1 * 1e3, per_circuit_wire_ms=t2 * 1e3, mixed_decoded_ms=t3 * 1e3,
                 mixed_wire_per_s=tot / t1, per_circuit_wire_per_s=tot / t2, mixed_decoded_per_s=tot / t3, speedup_over_per_circuit=t2 / t1,
                 reps=args.reps, window_bits=args.window_bits, pool=args.pool, screen_batch=gpu.get_option("screen_batch"),
                 stream_lanes=gpu.get_option("stream_lanes"))
    if "M3" in which:
        # 4 098 generators: the largest table window whose table fits the GPU is 8 (1.1 GB; 16 would take 137 GB, 20 1.8 TB), and
        # both sides of M3 use these tables
        capS, wS = 2048, 8
        gensS = gpu.gens_create(o.gens("G", capS), o.gens("H", capS), o.generator(), o.generator(), wS)
        psh = Pool(gpu, "shuffle1024", data["shuffle1024"])
        gs, al = psh.device(gpu, 1, rnd)
        allocs += al
        gr, al = p64.device(gpu, 4096, rnd)
        allocs += al
        pts, sc, ch, chi = psh.recs[0]
        shuffle_ok = []

        def separate():
            ok, _, _ = gpu.r1cs_verify_batch_param(gensS, psh.circ, 1, psh.n1, psh.k, psh.m, pts, sc, ch, chi, False, False)
            shuffle_ok.append(ok[0])
            return screened_one(gpu, gensS, gr)
        ta, tb = ab(gpu, lambda: gpu.r1cs_verify_mixed_screened_dev(gensS, [gs, gr]), separate, args.reps)
        all_ok(gpu, [gs, gr])
        assert set(shuffle_ok) == {1}
        emit(metric="M3", proofs=4097, mixed_ms=ta * 1e3, separate_ms=tb * 1e3, speedup=tb / ta, reps=args.reps, window_bits=wS, pool=1,
             note="separate = bpgpu_r1cs_verify_batch_param (host operands) for the shuffle + bpgpu_r1cs_verify_screened_dev for the ranges")
    for a in allocs:
        gpu.free(a)
    gpu.close()


LIB = lib_hash()

if __name__ == "__main__":
    main()
