#!/usr/bin/env python3
"""bench.py -- range-proof verifications/s (+ R1CS constraints/s of the prover) on MI355X: BASELINE.json's metric.

One step = one pass of the verification hot path (reference src/r1cs/verifier.rs:457-553: constraint flattening, inversions,
verifier scalar assembly, the 154-term mega_check MSM, identity test) over a batch of 1024 proofs of the 64-bit range gadget
(tests/r1cs.rs:620-652, m = 1: BASELINE configs[1]), inputs resident in HBM (proof points / scalars + host-transcript
challenges, boundary byte encodings of include/bpgpu.h).  Multi-GPU: one process per GPU, each rank verifies its own 1024
proofs per step (independent units, no data-path collective) -> weak scaling; value = all ranks' proofs / max-over-ranks time.
`python bench.py --gpus N` without a launcher starts the N rank processes itself (fresh children, before this process touches
the GPU); under torch.distributed.run it reads RANK / WORLD_SIZE.

Prints ONE JSON line on rank 0.  A plain run measures the headline only: it sets up, warms up, times --steps steps, writes
the last step's outputs if --dump-outputs is given and prints the line (`value`, `ms_per_step`, ...).  --full adds every
other measurement: `roofline` and `cpu_baseline`, the replay of one batch, the kernel timing regions, the secondary
verification legs, the other half of the metric -- the object `r1cs_prove` (configs[2]: 256 provers x (16 x 64 bit)), with
its own `roofline` and `cpu_baseline` -- and `shuffle_2e14` (configs[3] on one GPU); in a plain run those keys are null.

--dump-outputs DIR: after the timed steps, the per-proof accept bits of the timed region's last step (what a caller of
bpgpu_r1cs_verify_batch_dev receives) as DIR/accept_bits.npy, float32 (DIR/accept_bits_rank<r>.npy on rank r > 0).  The
workload is generated from fixed seeds, so the same arguments give the same inputs and the same last batch in every run.
"""
import argparse
import hashlib
import json
import multiprocessing as mp
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_BITS = 64
LABEL = b"RangeProofTest"
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
# Mix-weighted VALU issue peak: 74 % of the instructions of the elliptic-curve kernels are v_mad_i64_i32, which holds a
# SIMD for 4.6 cycles per wave64 instruction (33.9 T lane-MAD/s measured chip-wide, profiles/r01_microbench_primitives.log);
# the doubling / mixed-addition micro-benchmarks, which ARE this mix, issue one wave64 instruction per 4.25 cycles per
# SIMD at 8 waves/SIMD.  Per SIMD: 2.4 GHz / 4.25; the chip has 1024 SIMDs.  (A kernel of plain 2-cycle VALU instructions
# would exceed it.)
SIMD_ISSUE_PEAK_MIX = 2.4e9 / 4.25
N_SIMD = 256 * 4
VALU_ISSUE_PEAK_MIX = N_SIMD * SIMD_ISSUE_PEAK_MIX
MAD_PEAK_TOPS = 33.9            # measured v_mad_u64_u32 rate on MI355X (profiles/r01_microbench_primitives.log)
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_constants.json")
# configs[2]: 256 provers, each range-proving 16 x 64-bit values in one constraint system
P_NB, P_NVALS = 256, 16
P_N, P_Q = P_NVALS * N_BITS, P_NVALS * (2 * N_BITS + 1)


def _gen_workload(path, nb, seed0, nbatches=1):
    """child process (forked before the parent touches the GPU): prove nbatches x nb single-value 64-bit range proofs -- every
    one a DIFFERENT proof (its own value, blinding factors, hence challenges and verification scalars) -- with the product path
    itself (C++ host mirror over the C ABI, provers in lock-step on the GPU), replay the verifier transcripts on the host and
    write the operands of bpgpu_r1cs_verify_batch: batch 0 with everything the secondary legs need to `path` (a pickle), the
    points / scalars / challenges of ALL batches, batch-major, to `path`.pts / .sc / .ch (raw bytes)."""
    import ctypes as C
    import pickle
    host = C.CDLL(os.path.join(ROOT, "tests", "host", "libbph_capi.so"))
    lab = (C.c_uint8 * len(LABEL)).from_buffer_copy(LABEL)
    k = N_BITS.bit_length() - 1
    nvar = 11 + 1 + 2 * k
    cap = 8 * N_BITS + 8
    tmp = path + f".tmp{os.getpid()}"
    files = {e: open(tmp + e, "wb") for e in (".pts", ".sc", ".ch")}
    digests = set()
    t_gen = time.perf_counter()
    first = None
    for b in range(nbatches):
        vals = [(0x9E3779B97F4A7C15 * (b * nb + i + 1) + seed0) & ((1 << N_BITS) - 1) for i in range(nb)]
        arr = (C.c_uint64 * nb)(*vals)
        proofs, coms, plen = (C.c_uint8 * (nb * 4096))(), (C.c_uint8 * (nb * 64))(), C.c_size_t(0)
        for rep in range(2 if b == 0 else 1):      # batch 0: the second call has its workspaces and generator tables in place -- that one is timed
            t0 = time.perf_counter()
            rc = host.bph_range_prove_batch(C.c_size_t(nb), C.c_size_t(1), C.c_size_t(N_BITS), lab, C.c_size_t(len(LABEL)), arr,
                                            C.c_uint64(seed0 + b * nb), C.c_size_t(N_BITS), proofs, C.byref(plen), coms)
            if b == 0:
                prove_s = time.perf_counter() - t0
            assert rc == 0, f"bph_range_prove_batch rc={rc}"
        pl = plen.value
        pts, sc, ch = (C.c_uint8 * (nb * nvar * 64))(), (C.c_uint8 * (nb * 5 * 32))(), (C.c_uint8 * (nb * (6 + k) * 32))()
        init, dims = (C.c_uint8 * 32)(), (C.c_size_t * 6)()
        rp, kind, idx, coeff = (C.c_uint32 * (2 * N_BITS + 2))(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint8 * (32 * cap))()
        rc = host.bph_range_verify_inputs(C.c_size_t(nb), C.c_size_t(N_BITS), lab, C.c_size_t(len(LABEL)), coms, proofs,
                                          C.c_size_t(pl), C.c_size_t(N_BITS), pts, sc, ch, init, dims, rp, kind, idx, coeff)
        assert rc == 0, f"bph_range_verify_inputs rc={rc}"
        files[".pts"].write(pts)
        files[".sc"].write(sc)
        files[".ch"].write(ch)
        digests.add(hashlib.sha256(bytes(ch)).digest())
        if b == 0:
            first = (proofs, coms, pl, pts, sc, ch, init, dims, rp, kind, idx, coeff)
    gen_s = time.perf_counter() - t_gen
    assert len(digests) == nbatches, "the generated batches are not all different"
    for e, f in files.items():
        f.close()
        os.replace(tmp + e, path + e)
    proofs, coms, pl, pts, sc, ch, init, dims, rp, kind, idx, coeff = first
    n1, n, kk, m, q, nnz = list(dims)
    assert kk == k and m == 1
    G, H, B = (C.c_uint8 * (64 * N_BITS))(), (C.c_uint8 * (64 * N_BITS))(), (C.c_uint8 * 64)()
    assert host.bph_gens(ord("G"), 0, C.c_size_t(N_BITS), G) == 0 and host.bph_gens(ord("H"), 0, C.c_size_t(N_BITS), H) == 0
    host.bph_generator(B)
    # the same proofs in the reference's wire format (R1CSProof::to_bytes) + compressed commitments
    wire, wl_len = (C.c_uint8 * 4096)(), C.c_size_t(0)
    wires = []
    for i in range(nb):
        one = (C.c_uint8 * pl).from_buffer_copy(bytes(proofs)[i * pl:(i + 1) * pl])
        assert host.bph_proof_flat_to_wire(one, C.c_size_t(pl), wire, C.byref(wl_len)) == 0
        wires.append(bytes(wire)[:wl_len.value])
    ccom = (C.c_uint8 * (nb * 32))()
    assert host.bph_compress_points(coms, C.c_size_t(nb), ccom) == 0
    wl = {"wire_proofs": b"".join(wires), "wire_len": len(wires[0]), "wire_commitments": bytes(ccom),
          "proofs": bytes(proofs)[:nb * pl], "proof_len": pl, "commitments": bytes(coms), "points": bytes(pts),
          "scalars": bytes(sc), "challenges": bytes(ch), "init_state": bytes(init), "dims": (n1, n - n1, k, m),
          "csr": (list(rp)[:q + 1], list(kind)[:nnz], list(idx)[:nnz], bytes(coeff)[:32 * nnz]),
          "G": bytes(G), "H": bytes(H), "B": bytes(B), "prove_seconds": prove_s, "nbatches": nbatches, "gen_seconds": gen_s}
    with open(tmp, "wb") as f:
        pickle.dump(wl, f)
    os.replace(tmp, path)


def _load_many(cache, wl):
    """points / scalars / challenges of ALL generated batches (batch-major raw bytes) and their number"""
    out = []
    for e in (".pts", ".sc", ".ch"):
        with open(cache + e, "rb") as f:
            out.append(f.read())
    nbat = wl.get("nbatches", 1)
    assert len(out[0]) == nbat * len(wl["points"]) and out[1][:len(wl["scalars"])] == wl["scalars"]
    return out[0], out[1], out[2], nbat


def _tampered_batch(pts, sc, ch, nb, nvar):
    """batch 0 with four proofs made invalid in four different ways -> (points, scalars, challenges, expected accept bits):
    t_x off by one, a challenge flipped, a proof point replaced by another proof's, an off-curve point"""
    pts, sc, ch = bytearray(pts), bytearray(sc), bytearray(ch)
    bad = sorted({3 % nb, nb // 3, (2 * nb) // 3 + 1, nb - 1})
    ways = ("t_x", "challenge", "foreign_point", "off_curve")
    cl = len(ch) // nb
    for w, i in zip(ways, bad):
        if w == "t_x":
            sc[i * 160] ^= 1
        elif w == "challenge":
            ch[i * cl + 32] ^= 2
        elif w == "foreign_point":
            j = (i + 1) % nb
            pts[i * nvar * 64 + 64:i * nvar * 64 + 128] = pts[j * nvar * 64 + 64:j * nvar * 64 + 128]
        else:
            pts[i * nvar * 64 + 32] ^= 1          # y of the first point: (x, y ^ 1) is not on the curve
    exp = b"".join((0 if i in bad else 1).to_bytes(4, "little") for i in range(nb))
    return bytes(pts), bytes(sc), bytes(ch), exp


# ---- CPU legs: the oracle (tests/oracle_lib.py -> oracle/liboracle.so) runs ONLY inside these three worker functions, in
# processes forked before this process initialises the GPU
def _cpu_verify_chunk(args):
    import oracle_lib as o
    proofs, coms, plen = args
    nb = len(proofs) // plen
    t0 = time.perf_counter()
    ok = o.r1cs_verify_many(o.K_RANGE, N_BITS, LABEL, [], coms, 1, proofs, plen, nb, N_BITS)
    return sum(ok), time.perf_counter() - t0


def _cpu_prove_chunk(args):
    """`count` provers of configs[2]'s circuit (16 x 64-bit range gadgets in one constraint system) on the CPU oracle"""
    import oracle_lib as o
    seed, count = args
    param = N_BITS | (P_NVALS << 16)
    t0 = time.perf_counter()
    n_ok = 0
    for j in range(count):
        vals = [((0x9E3779B97F4A7C15 * (i + 1 + 31 * (seed + j))) & ((1 << 64) - 1)) for i in range(P_NVALS)]
        rc, proof, com = o.r1cs_prove(o.K_RANGE_MULTI, param, LABEL, vals, 9000 + seed + j, P_N)
        n_ok += rc == 0
    dt = time.perf_counter() - t0
    return n_ok, dt


def _cpu_check_proofs(args):
    """the CPU oracle's verdict on proofs made by the GPU prover inside a timed region: (kind, param, label, commitments, proof, cap)"""
    import oracle_lib as o
    return [o.r1cs_verify(kind, param, label, [], com, proof, cap) for kind, param, label, com, proof, cap in args]


def _cpu_baseline(pool, nworkers, wl, nb):
    """The CPU oracle's Verifier::verify restatement (transcript replay + scalar assembly + 154-term Pippenger MSM) on a
    bounded sample of the same workload: all host cores, then ONE process; then its Prover::prove restatement, one prover of
    configs[2]'s circuit per core."""
    plen = wl["proof_len"]
    per = (nb + nworkers - 1) // nworkers
    chunks = []
    for c in range(nworkers):
        lo, hi = c * per, min(nb, (c + 1) * per)
        if hi > lo:
            chunks.append((wl["proofs"][lo * plen:hi * plen], wl["commitments"][64 * lo:64 * hi], plen))
    pool.map(_cpu_verify_chunk, [(b"", b"", plen)] * nworkers)     # start the workers, load the library
    t0 = time.perf_counter()
    res = pool.map(_cpu_verify_chunk, chunks, chunksize=1)
    wall = time.perf_counter() - t0
    assert sum(r[0] for r in res) == nb, "the CPU oracle rejects proofs made by the GPU prover"
    allc = {"value": nb / wall, "unit": "verifications/s", "cores": len(chunks), "kind": "port",
            "sample": f"{nb} proofs of the same workload, oracle cs_verify = the WHOLE of Verifier::verify (transcript replay "
                      f"+ scalar assembly + 154-term Pippenger MSM), {len(chunks)} processes, {sum(r[1] for r in res):.1f} s CPU; "
                      "the like-for-like GPU figure is `with_device_transcript`, not `value` (whose challenges are inputs)"}
    n1 = min(nb, 128)
    t0 = time.perf_counter()
    r1 = pool.map(_cpu_verify_chunk, [(wl["proofs"][:n1 * plen], wl["commitments"][:64 * n1], plen)])
    wall1 = time.perf_counter() - t0
    assert r1[0][0] == n1
    one = {"value": n1 / wall1, "unit": "verifications/s", "cores": 1, "kind": "port",
           "sample": f"the first {n1} proofs of the same workload, one process (BASELINE.md's single-thread column)"}
    t0 = time.perf_counter()
    rp = pool.map(_cpu_prove_chunk, [(w, 1) for w in range(nworkers)], chunksize=1)
    wallp = time.perf_counter() - t0
    assert sum(r[0] for r in rp) == nworkers
    prove = {"value": nworkers * P_Q / wallp, "unit": "R1CS constraints/s", "cores": nworkers, "kind": "port",
             "proofs_per_s": nworkers / wallp,
             "sample": f"{nworkers} provers of the same circuit (16 x 64-bit range gadgets, q = {P_Q}), one per process, the oracle's "
                       f"Prover::prove restatement (prover.rs:412-727 incl. InnerProductProof::create), {sum(r[1] for r in rp):.1f} s CPU; "
                       f"one process alone: {P_Q / max(r[1] for r in rp):.0f} constraints/s"}
    return allc, one, prove


def _one_call_child(cache, window_bits):
    """A process of its own, as a caller of the library would be: ONE context, ONE call (bpgpu_r1cs_verify_stream_dev /
    bpgpu_r1cs_verify_stream) over many batches; the library owns the ring of lanes and the hardware-queue setting.  Prints a JSON
    object.  (Inside the main process the 20 contexts of the timed region hold hardware queues of their own: 40 streams on 24
    queues make the lanes share queues with them.)"""
    import pickle
    import torch  # noqa: F401  (the same import order as a torch-using host; nothing here touches the GPU through torch)
    import mpc_bulletproof_amd as mb
    with open(cache, "rb") as f:
        wl = pickle.load(f)
    n1, n2, k, m = wl["dims"]
    pts, sc, ch = wl["points"], wl["scalars"], wl["challenges"]
    nb = len(sc) // 160
    pts_all, sc_all, ch_all, nbat = _load_many(cache, wl)

    def many(buf_all, one, reps):
        """`reps` batches of the workload, all different when it holds that many (else the cycle repeated)"""
        return buf_all[:reps * len(one)] if reps <= nbat else (buf_all * ((reps + nbat - 1) // nbat))[:reps * len(one)]

    all_ok = (1).to_bytes(4, "little") * nb
    gpu = mb.BpGpu(int(os.environ.get("LOCAL_RANK", "0")))
    circ = gpu.circuit_create(*wl["csr"], n1 + n2, m)
    gens = gpu.gens_create(wl["G"], wl["H"], wl["B"], wl["B"], window_bits)
    out = {}
    for tag, reps in (("20k", 20), ("64k", 64), ("256k", 256)):
        d_p2, d_s2, d_c2 = gpu.to_device(many(pts_all, pts, reps)), gpu.to_device(many(sc_all, sc, reps)), gpu.to_device(many(ch_all, ch, reps))
        d_o2 = gpu.malloc(4 * nb * reps)
        ts = []
        for rep_ in range(8):
            gpu.sync()
            t0 = time.perf_counter()
            gpu.r1cs_verify_stream_dev(gens, circ, nb * reps, n1, k, d_p2, d_s2, d_c2, d_o2)
            gpu.sync()
            ts.append(time.perf_counter() - t0)
        assert gpu.download(d_o2, 4 * nb * reps) == all_ok * reps
        for d in (d_p2, d_s2, d_c2, d_o2):
            gpu.free(d)
        ts = sorted(ts[2:])
        out[tag] = {"value": nb * reps / ts[len(ts) // 2], "unit": "verifications/s", "proofs": nb * reps, "ms_per_call": ts[len(ts) // 2] * 1e3,
                    "best_ms": ts[0] * 1e3}
    # ... per-proof accept bits through the SCREENED call: the combined check of every batch first, the per-proof path only for a
    # batch that fails it.  All proofs valid (the service's usual case), and with ONE tampered proof in the whole call.
    import random as _random
    rnd_ = _random.Random(0x5C2EE)
    ORDER_N = 0x0800000000000010ffffffffffffffffb781126dcae7b2321e66a241adc64d2f
    rho1 = b"".join(rnd_.randrange(1, ORDER_N).to_bytes(32, "little") for _ in range(nb))
    screened = {}
    for tag, reps in (("20k", 20), ("256k", 256)):
        d_p2, d_s2, d_c2, d_r2 = (gpu.to_device(many(pts_all, pts, reps)), gpu.to_device(many(sc_all, sc, reps)), gpu.to_device(many(ch_all, ch, reps)),
                                  gpu.to_device(rho1 * reps))
        d_o2 = gpu.malloc(4 * nb * reps)
        ts = []
        for rep_ in range(8):
            gpu.sync()
            t0 = time.perf_counter()
            nfall = gpu.r1cs_verify_screened_dev(gens, circ, nb * reps, n1, k, d_p2, d_s2, d_c2, d_r2, d_o2)
            gpu.sync()
            ts.append(time.perf_counter() - t0)
            assert nfall == 0
        assert gpu.download(d_o2, 4 * nb * reps) == all_ok * reps
        ts = sorted(ts[2:])
        screened[tag] = {"value": nb * reps / ts[len(ts) // 2], "unit": "verifications/s", "proofs": nb * reps, "ms_per_call": ts[len(ts) // 2] * 1e3}
        if tag == "256k":      # one proof with t_x off by one: its screening batch (only) is verified proof by proof
            bad_i = 100 * nb + 517
            sc_bad = bytearray(many(sc_all, sc, reps))
            sc_bad[bad_i * 160] ^= 1
            gpu.free(d_s2)
            d_s2 = gpu.to_device(bytes(sc_bad))
            ts = []
            for rep_ in range(5):
                gpu.sync()
                t0 = time.perf_counter()
                nfall = gpu.r1cs_verify_screened_dev(gens, circ, nb * reps, n1, k, d_p2, d_s2, d_c2, d_r2, d_o2)
                gpu.sync()
                ts.append(time.perf_counter() - t0)
                assert nfall == 1
            got = gpu.download(d_o2, 4 * nb * reps)
            assert got == all_ok * 100 + all_ok[:4 * 517] + bytes(4) + all_ok[4 * 518:] + all_ok * (reps - 101)
            ts = sorted(ts[1:])
            screened["256k_one_bad_proof"] = {"value": nb * reps / ts[len(ts) // 2], "unit": "verifications/s", "ms_per_call": ts[len(ts) // 2] * 1e3,
                                              "fallback_batches": 1}
        for d in (d_p2, d_s2, d_c2, d_r2, d_o2):
            gpu.free(d)
    # ... and the whole Verifier::verify that way: transcript on the device per batch, then the combined check
    reps = 256
    d_i2, d_p2, d_s2, d_r2 = (gpu.to_device(wl["init_state"] * (nb * reps)), gpu.to_device(many(pts_all, pts, reps)), gpu.to_device(many(sc_all, sc, reps)),
                              gpu.to_device(rho1 * reps))
    d_o2 = gpu.malloc(4 * nb * reps)
    ts = []
    for rep_ in range(7):
        gpu.sync()
        t0 = time.perf_counter()
        nfall = gpu.r1cs_verify_screened_fs_dev(gens, circ, nb * reps, n1, k, d_i2, d_p2, d_s2, d_r2, d_o2)
        gpu.sync()
        ts.append(time.perf_counter() - t0)
        assert nfall == 0
    assert gpu.download(d_o2, 4 * nb * reps) == all_ok * reps
    for d in (d_i2, d_p2, d_s2, d_r2, d_o2):
        gpu.free(d)
    ts = sorted(ts[2:])
    screened["256k_with_device_transcript"] = {"value": nb * reps / ts[len(ts) // 2], "unit": "verifications/s", "ms_per_call": ts[len(ts) // 2] * 1e3,
                                               "note": "bpgpu_r1cs_verify_screened_fs_dev: the whole Verifier::verify (transcript replay on the device) -- "
                                                       "the figure to hold against cpu_baseline when per-proof verdicts are wanted"}
    screened["note"] = ("bpgpu_r1cs_verify_screened_dev: per-proof accept bits; every batch of 2560 proofs is first checked as ONE combined point "
                        "(random weights), only a batch that fails is verified proof by proof.  The verdicts are those of the per-proof call")
    out["screened"] = screened
    # ... and the same from page-locked HOST memory: every batch's upload and verdict download ride on its lane
    reps = 64
    h_p, h_s, h_c = (mb.lib.host_alloc(len(pts) * reps, many(pts_all, pts, reps)), mb.lib.host_alloc(len(sc) * reps, many(sc_all, sc, reps)),
                     mb.lib.host_alloc(len(ch) * reps, many(ch_all, ch, reps)))
    ts = []
    for rep_ in range(6):
        gpu.sync()
        t0 = time.perf_counter()
        ok_h = gpu.r1cs_verify_stream(gens, circ, nb * reps, n1, k, m, h_p, h_s, h_c, raw=True)
        ts.append(time.perf_counter() - t0)
        assert ok_h == all_ok * reps
    ts = sorted(ts[2:])
    out["host_64k"] = {"value": nb * reps / ts[len(ts) // 2], "unit": "verifications/s", "proofs": nb * reps, "ms_per_call": ts[len(ts) // 2] * 1e3,
                       "bytes_uploaded": (len(pts) + len(sc) + len(ch)) * reps}
    out["distinct_batches"] = nbat
    out["hw_queues_exported_by_the_caller"] = os.environ.get("GPU_MAX_HW_QUEUES")     # None: the library's own default is in force
    out["note"] = ("bpgpu_r1cs_verify_stream(_dev) in a process of its own: one context, one call, no environment variable exported by the caller; the "
                   "library owns the ring of 20 lanes.  20k = a burst of 20 batches on an idle GPU (the first front launches and the last back launches "
                   "have the chip to themselves); 64k / 256k approach the steady state; host_64k takes the operands from page-locked host memory "
                   "and returns the verdicts there (SURVEY 8d's metric as written).  Median of 6 (4) calls")
    print(json.dumps(out), flush=True)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N rank processes (fresh interpreters; this parent never
    initialises the GPU) with the rendezvous environment torch.distributed.run would give them, relay rank 0's stdout."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        while any(p.poll() is None for p in procs):
            failed = [p.returncode for p in procs if p.poll() not in (None, 0)]
            if failed:                      # the other ranks would wait for the dead one in the next collective
                rc = abs(failed[0])
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=20)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    sys.exit(max([rc] + [abs(p.returncode or 0) for p in procs]) if rc == 0 else rc)


def _lib_hash():
    h = hashlib.sha256()
    with open(os.path.join(ROOT, "mpc_bulletproof_amd", "libbpgpu.so"), "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()[:16]


def _union_ms(intervals):
    """total length of the union of (start, end) intervals"""
    busy, cs, ce = 0.0, None, None
    for a, b in sorted(intervals):
        if ce is None or a > ce:
            if ce is not None:
                busy += ce - cs
            cs, ce = a, b
        elif b > ce:
            ce = b
    return busy + (ce - cs if ce is not None else 0.0)


def main():
    # Steps in flight: the main region rotates over `inflight` independent contexts (a stream + workspaces each).  The HIP runtime
    # maps streams onto GPU_MAX_HW_QUEUES hardware queues; libbpgpu.so sets 24 when it is loaded (unless the process chose a
    # value), and this script loads it before torch initialises HIP.  One stream per context.
    os.environ.setdefault("BPGPU_SINGLE_STREAM", "1")
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--window-bits", type=int, default=int(os.environ.get("BPGPU_WINDOW_BITS", "20")),
                    help="window of the resident generator tables: 20 bits = 13 table additions per generator term, a 57 GB "
                         "table for the 130 generators of the 64-bit gadget (16 bits: 16 additions, 4.5 GB)")
    ap.add_argument("--inflight", type=int, default=int(os.environ.get("BPGPU_INFLIGHT", "20")),
                    help="steps in flight: consecutive steps alternate between this many independent contexts "
                         "(streams + workspaces), so the kernels of several batches overlap on the GPU")
    ap.add_argument("--distinct-batches", type=int, default=int(os.environ.get("BPGPU_DISTINCT_BATCHES", "256")),
                    help="number of DIFFERENT batches of proofs the workload holds; the timed region (and the one-call legs) cycle "
                         "through them, so the fixed-base table rows a step gathers (110 MB of a 57 GB table) are never the rows of "
                         "a recent step: 256 batches touch 28 GB of rows per cycle against 256 MiB of Infinity Cache")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run every other measurement: CPU baselines, the one-batch replay, kernel timing "
                         "(rooflines), the secondary verification legs, the prover and the shuffle (the --no-* options trim it)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the accept bits of the timed region's last step to DIR/accept_bits.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-combined", action="store_true", help="with --full: skip the secondary verification measurements (one-call "
                                                               "stream, H2D-inclusive, device transcript, wire format, combined batch "
                                                               "check, single batch)")
    ap.add_argument("--no-prover", action="store_true", help="with --full: skip the R1CS prover measurements (N = 1 only)")
    ap.add_argument("--prover-threads", type=int, default=3, help="worker threads (one context each) of the prover stream")
    ap.add_argument("--prover-batches", type=int, default=12, help="batches of 256 provers in the timed prover stream")
    ap.add_argument("--workload-cache", default=None,
                    help="pickle of the generated workload (written if absent); lets a profiled run skip the fork pool")
    ap.add_argument("--one-call-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.one_call_child:
        _one_call_child(a.one_call_child, a.window_bits)
        return

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _spawn_ranks(a.gpus)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus != world:
        print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus} "
              f"or let bench.py start the ranks itself (no WORLD_SIZE in the environment)", file=sys.stderr)
        sys.exit(2)
    nb = a.batch

    # ---- synthetic workload (setup, untimed), generated by the product path itself in a child process forked before
    # this process touches the GPU.  Every rank verifies the same batch (weak scaling): local rank 0 generates it
    # once and publishes it through a file, the other ranks wait for the file.  The CPU baselines (the oracle's
    # restatement) run in a fork pool on rank 0, created before any GPU initialisation here and kept for the oracle's
    # verdict on proofs the GPU prover makes later.
    import pickle
    import tempfile
    ncpu = max(1, min(os.cpu_count() or 1, 32))
    seed0 = 0xB0117E7
    nbat_req = max(1, a.distinct_batches)
    cache = f"{a.workload_cache}.{nb}" if a.workload_cache else os.path.join(
        tempfile.gettempdir(), f"bpgpu_workload_{os.environ.get('MASTER_PORT', 'solo')}_{os.getppid()}_{nb}x{nbat_req}.pkl")
    if a.workload_cache and os.path.exists(cache) and local_rank == 0:      # a cached workload with fewer batches than asked for is made again
        with open(cache, "rb") as f:
            if pickle.load(f).get("nbatches", 1) < nbat_req:
                os.remove(cache)
    if not os.path.exists(cache) and local_rank == 0:
        child = mp.get_context("fork").Process(target=_gen_workload, args=(cache, nb, seed0, max(1, a.distinct_batches)))
        child.start()
        child.join()
        if child.exitcode != 0:
            raise RuntimeError(f"workload generation failed (exit code {child.exitcode}): the HIP path is required, "
                               "there is no CPU fallback")
    deadline = time.time() + 1200
    while not os.path.exists(cache):
        if time.time() > deadline:
            raise RuntimeError("workload file never appeared")
        time.sleep(0.5)
    with open(cache, "rb") as f:
        wl = pickle.load(f)
    cpu = cpu1 = cpu_prove = None
    pool = None
    if rank == 0 and a.full and not a.no_cpu_baseline:
        pool = mp.get_context("fork").Pool(ncpu)
        cpu, cpu1, cpu_prove = _cpu_baseline(pool, ncpu, wl, nb)
    n1, n2, k, m = wl["dims"]
    rp, kind, idx, coeff = wl["csr"]
    pts, sc, ch = wl["points"], wl["scalars"], wl["challenges"]
    # ---- secondary: the one-call entry point, measured in a fresh process BEFORE this one takes the GPU (one after the other)
    one_call = None
    if a.full and rank == 0 and world == 1 and not a.no_combined and nb == 1024:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-call-child", cache, "--window-bits", str(a.window_bits)],
                           capture_output=True, text=True, timeout=600, env={k_: v for k_, v in os.environ.items() if k_ != "GPU_MAX_HW_QUEUES"})
        if r.returncode != 0:      # a secondary leg: reported in its place (and on stderr), the headline line survives
            print("bench.py: the one-call child failed:\n" + r.stderr[-2000:], file=sys.stderr)
            one_call = {"error": "the one-call child process failed: " + r.stderr.strip().splitlines()[-1][:300] if r.stderr.strip() else "no output"}
        else:
            one_call = json.loads(r.stdout.strip().splitlines()[-1])

    # ---- GPU
    import torch                         # (first, so that libbpgpu.so binds to the HIP runtime torch ships; neither import touches the GPU)
    import torch.distributed as dist
    import mpc_bulletproof_amd as mb     # loads libbpgpu.so, which sets the hardware-queue default before the first HIP call
    if world > 1:
        if os.environ.get("BPGPU_BENCH_REHEARSAL"):
            # control-flow rehearsal of the multi-rank path on a ONE-GPU box: all ranks share device 0, gloo instead
            # of RCCL (NCCL refuses two ranks on one device).  Not a measurement.
            dev = 0
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
        else:
            dev = local_rank
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        dev = local_rank
    ctxs = [mb.BpGpu(dev) for _ in range(max(1, a.inflight))]
    gpu = ctxs[0]
    circ = gpu.circuit_create(rp, kind, idx, coeff, n1 + n2, m)
    gens = gpu.gens_create(wl["G"], wl["H"], wl["B"], wl["B"], a.window_bits)
    import ctypes as C_
    # every step verifies a DIFFERENT batch of the workload (cycling through `nbat` of them; rank r starts a share of the cycle
    # further on): the table rows a step gathers are not the rows of any recent step
    pts_all, sc_all, ch_all, nbat = _load_many(cache, wl)
    d_pts_all, d_sc_all, d_ch_all = gpu.to_device(pts_all), gpu.to_device(sc_all), gpu.to_device(ch_all)
    lp, ls, lc = len(pts), len(sc), len(ch)

    def batch_ptrs(j):
        j %= nbat
        return (C_.c_void_p(d_pts_all.value + j * lp), C_.c_void_p(d_sc_all.value + j * ls), C_.c_void_p(d_ch_all.value + j * lc))

    d_pts, d_sc, d_ch = batch_ptrs(0)
    d_oks = [gpu.malloc(4 * nb) for _ in ctxs]
    counter = [0]
    rank_off = (rank * nbat) // max(1, world)
    all_ok = (1).to_bytes(4, "little") * nb
    # untimed pre-check of the exact launches the timed region runs, on a batch that holds INVALID proofs (a verdict kernel that
    # always wrote 1 would pass the all-ones checks below): accept bits against the expected pattern, on every context
    nvar_ = 11 + m + 2 * k
    t_pts, t_sc, t_ch, t_exp = _tampered_batch(pts, sc, ch, nb, nvar_)
    d_tp, d_ts, d_tc = gpu.to_device(t_pts), gpu.to_device(t_sc), gpu.to_device(t_ch)
    for c, d in zip(ctxs, d_oks):
        c.r1cs_verify_batch_dev(gens, circ, nb, n1, k, d_tp, d_ts, d_tc, d)
    for c, d in zip(ctxs, d_oks):
        c.sync()
        assert c.download(d, 4 * nb) == t_exp, "GPU verification: wrong accept bits on the batch with tampered proofs"
        c.input_flag()
    for d in (d_tp, d_ts, d_tc):
        gpu.free(d)

    def step():
        i = counter[0] % len(ctxs)
        p_, s_, c_ = batch_ptrs(counter[0] + rank_off)
        counter[0] += 1
        ctxs[i].r1cs_verify_batch_dev(gens, circ, nb, n1, k, p_, s_, c_, d_oks[i])

    def step_same():
        i = counter[0] % len(ctxs)
        counter[0] += 1
        ctxs[i].r1cs_verify_batch_dev(gens, circ, nb, n1, k, d_pts, d_sc, d_ch, d_oks[i])

    def sync_all():
        # one device-wide synchronisation (the contexts' streams are ordinary blocking HIP streams of this device);
        # a hipStreamSynchronize per context costs ~0.15 ms each on an idle stream
        torch.cuda.synchronize()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, steps, before=None):
        """EXACTLY `steps` calls of fn(i) between two fences; max over ranks.  The GPU is handed over BUSY: a burst of one
        un-timed call per context runs right up to the opening fence (result checks, profile reads and buffer setup before a
        leg leave the device idle for milliseconds, and an idle device starts the first kernels of a short run slowly);
        `before()` runs between that burst's completion and the fence (switches event timing on: a flag, no GPU work)."""
        # A SHORT run (the driver's 20 steps) is a burst on an idle GPU, and how fast a burst runs depends on what the GPU did just
        # before: right after the continuous warm-up 3.5-3.8 M/s, after an idle pause of 2 ms .. 1 s 2.3-3.3 M/s, after n untimed
        # bursts of the same shape 3.6 / 3.8 / 3.9 / 4.0-4.1 M/s for n = 1 / 2 / 4 / 8 (profiles/r04_burst_precondition.log: the
        # clocks settle on the load pattern).  So the untimed lead-in of a short run is the timed region's own pattern -- `steps`
        # calls, then a synchronisation -- repeated BPGPU_WARM_BURSTS times (8; 0 = one call per context, the lead-in of long runs).
        lead = int(os.environ.get("BPGPU_WARM_BURSTS", "8")) if steps <= 256 else 0
        for _ in range(lead):
            for i in range(steps):
                fn(i)
            sync_all()
        if not lead:
            for i in range(len(ctxs)):
                fn(i)
            sync_all()
        if before:
            before()
        fence()
        t0 = time.perf_counter()
        for i in range(steps):
            fn(i)
        sync_all()
        fence()
        dt = time.perf_counter() - t0
        if world > 1:
            from mpc_bulletproof_amd import sharding
            dt = sharding.max_over_ranks(dt)
        return dt

    for _ in range(max(a.warmup, len(ctxs))):
        step()
    sync_all()
    for c, d in zip(ctxs, d_oks):
        assert c.download(d, 4 * nb) == all_ok and c.input_flag() == 0, "GPU verification disagrees"
    # the checks above leave the GPU idle for milliseconds: the warm-up keeps submitting steps (untimed) for
    # BPGPU_WARM_SECONDS of wall time; timed() then hands the device over busy
    warm_s = float(os.environ.get("BPGPU_WARM_SECONDS", "0.3"))
    tw = time.perf_counter()
    while time.perf_counter() - tw < warm_s:
        for _ in range(2 * len(ctxs)):
            step()
    sync_all()
    counter[0] = 0
    # ======== the timed region: no event timing inside it
    dt = timed(lambda i: step(), a.steps)
    last = (counter[0] - 1) % len(ctxs)          # the context of the timed region's last step
    for j, (c, d) in enumerate(zip(ctxs, d_oks)):
        got = c.download(d, 4 * nb)
        assert got == all_ok
        if j == last:
            last_ok = got
    if a.dump_outputs:
        import numpy as np
        os.makedirs(a.dump_outputs, exist_ok=True)
        np.save(os.path.join(a.dump_outputs, "accept_bits.npy" if rank == 0 else f"accept_bits_rank{rank}.npy"),
                np.frombuffer(last_ok, dtype="<u4").astype(np.float32))
    # the same region REPLAYING one batch (what rounds 1-3 reported): its 110 MB of table rows stay in the Infinity Cache
    dt_same = None
    if a.full:
        counter[0] = 0
        dt_same = timed(lambda i: step_same(), a.steps)

    # ======== kernel timing, measured live with HIP events on the launch streams (bpgpu_profile_*), in two further regions:
    #   (1) the same K steps (at most 256) REPLAYED with an event pair around every launch of every context: the union of the
    #       intervals is the time the GPU was busy, the union per kernel kind the time that kernel was resident -- neither
    #       can exceed the wall clock; the plain averages ("residency") are what a launch lasts among its neighbours;
    #   (2) a few un-pipelined steps on one context: each kernel's SOLO duration -- what rocprofv3 of a solo run measures
    #       (profiles/, tools/profile_all.sh) and the only duration that belongs to the kernel alone.  `roofline` uses it.
    noprof = not a.full or bool(os.environ.get("BPGPU_BENCH_NOPROF"))
    replay = solo = None
    if not noprof:
        def all_on():
            for c in ctxs:
                c.profile_enable(True)

        epoch = gpu.profile_epoch()
        for c in ctxs:
            c.profile_read()
        counter[0] = 0
        replay_steps = min(a.steps, 256)
        rdt = timed(lambda i: step(), replay_steps, before=all_on)
        iv = []
        for c in ctxs:
            c.profile_enable(False)
            iv += c.profile_intervals(epoch)
        t_lo = min(x[1] for x in iv)
        t_hi = max(x[2] for x in iv)
        kinds = sorted({x[0] for x in iv})
        busy = _union_ms([(x[1], x[2]) for x in iv])
        replay = {"steps": replay_steps, "ms_per_step": rdt / replay_steps * 1e3,
                  "gpu_busy_ms_per_step": busy / replay_steps, "gpu_busy_frac": busy / (t_hi - t_lo),
                  "resident_ms_per_step": {n_: _union_ms([(x[1], x[2]) for x in iv if x[0] == n_]) / replay_steps for n_ in kinds},
                  "residency_avg_ms": {n_: sum(x[2] - x[1] for x in iv if x[0] == n_) / max(1, sum(1 for x in iv if x[0] == n_)) for n_ in kinds},
                  "launches": {n_: sum(1 for x in iv if x[0] == n_) for n_ in kinds},
                  "what": f"the same {replay_steps} steps again with a HIP-event pair around EVERY launch of every context (the pairs are "
                          "barriers in the queues: this region runs slower than the timed one).  gpu_busy = union of all launch "
                          "intervals; resident_ms_per_step[k] = union of kernel k's intervals / steps (<= ms_per_step by construction); "
                          "residency_avg_ms[k] = plain average of a launch's duration among its ~20 neighbours (not a roofline input)"}
        # (2) solo
        sync_all()
        gpu.profile_enable(True)
        solo_steps = 12
        for _ in range(solo_steps):
            gpu.r1cs_verify_batch_dev(gens, circ, nb, n1, k, d_pts, d_sc, d_ch, d_oks[0])
            gpu.sync()
        gpu.profile_enable(False)
        solo = {n_: (ms / cnt, cnt) for n_, (ms, cnt) in gpu.profile_read().items() if cnt}
        assert gpu.download(d_oks[0], 4 * nb) == all_ok

    fs = wire = comb = h2d = single = None
    if a.full and not a.no_combined:
        # ---- secondary: ONE batch at a time (no pipelining): the latency of a batch's kernel chain
        lat = []
        ctxs[0].set_latency_mode(True)      # the context-level hint for un-pipelined callers (include/bpgpu.h)
        for _ in range(9):
            sync_all()
            t0 = time.perf_counter()
            ctxs[0].r1cs_verify_batch_dev(gens, circ, nb, n1, k, d_pts, d_sc, d_ch, d_oks[0])
            ctxs[0].sync()
            lat.append(time.perf_counter() - t0)
        ctxs[0].set_latency_mode(False)
        assert ctxs[0].download(d_oks[0], 4 * nb) == all_ok
        lat = sorted(lat[2:])
        single = {"value": nb / lat[len(lat) // 2], "unit": "verifications/s", "ms_per_batch": lat[len(lat) // 2] * 1e3,
                  "min_ms": lat[0] * 1e3, "note": "one un-pipelined 1024-proof batch on an idle GPU, submit to host-visible completion "
                                                  "(median of 7, context in latency mode: bpgpu_set_latency_mode): front | scalars | windows | groups | back | verdict"}

        # ---- secondary: SURVEY 8d's metric as written -- the proof points, proof scalars and challenges of every step are
        # uploaded from page-locked host memory inside the timed region (asynchronous copies on the step's stream)
        lpk = lp + ls + lc                          # one page-locked staging buffer holding every batch packed, one asynchronous copy per step
        h_in = mb.lib.host_alloc(lpk * nbat, b"".join(pts_all[j * lp:(j + 1) * lp] + sc_all[j * ls:(j + 1) * ls] + ch_all[j * lc:(j + 1) * lc]
                                                      for j in range(nbat)))
        d_in = [c.malloc(lpk) for c in ctxs]

        def hstep(i):
            j = i % len(ctxs)
            c, dp = ctxs[j], d_in[j]
            c.upload_async(dp, h_in.value + ((i + rank_off) % nbat) * lpk, lpk)
            c.r1cs_verify_batch_dev(gens, circ, nb, n1, k, dp, C_.c_void_p(dp.value + lp), C_.c_void_p(dp.value + lp + ls),
                                    d_oks[j])

        for i in range(len(ctxs)):
            hstep(i)
        sync_all()
        for c, d in zip(ctxs, d_oks):
            assert c.download(d, 4 * nb) == all_ok
        hdt = timed(hstep, a.steps)
        h2d = {"value": world * nb * a.steps / hdt, "unit": "verifications/s", "ms_per_step": hdt / a.steps * 1e3,
               "bytes_per_step": lpk,
               "note": "as `value`, plus the upload of every step's proof points, proof scalars and challenges from page-locked "
                       "host memory inside the timed region (SURVEY 8d: 'incl. H2D of proof scalars + points').  The bench contract "
                       "defines `value` with inputs resident in HBM, so this PCIe-inclusive rate is reported here, beside it"}

        # ---- secondary: the same per-proof verification with the Fiat-Shamir transcript replayed on the device
        # (SURVEY 8f N1): inputs are the proofs + one 32-byte initial chain state per proof, no host challenges
        d_init = gpu.to_device(wl["init_state"] * nb)

        def fstep(i):
            j = i % len(ctxs)
            p_, s_, _c = batch_ptrs(i + rank_off)
            ctxs[j].r1cs_verify_batch_fs_dev(gens, circ, nb, n1, k, d_init, p_, s_, d_oks[j])

        for i in range(len(ctxs)):
            fstep(i)
        sync_all()
        for c, d in zip(ctxs, d_oks):
            assert c.download(d, 4 * nb) == all_ok
        fdt = timed(fstep, a.steps)
        fs = {"value": world * nb * a.steps / fdt, "unit": "verifications/s", "ms_per_step": fdt / a.steps * 1e3,
              "note": "whole Verifier::verify incl. the transcript replay (keccak256 chain, hash_to_scalar) on the GPU; "
                      "per-proof accept bits.  This is the figure to hold against cpu_baseline (same work)"}

        # ---- secondary: the same proofs taken in the reference's WIRE format (SURVEY 8f N3 + N1): unpack, decompress the
        # 25 points of every proof (a square root in F_p each), transcript, verification -- all on the device
        d_wp, d_wc = gpu.to_device(wl["wire_proofs"]), gpu.to_device(wl["wire_commitments"])

        def wstep(i):
            j = i % len(ctxs)
            ctxs[j].r1cs_verify_batch_wire_dev(gens, circ, nb, n1, wl["wire_len"], d_wp, d_wc, d_init, d_oks[j])

        for i in range(len(ctxs)):
            wstep(i)
        sync_all()
        for c, d in zip(ctxs, d_oks):
            assert c.download(d, 4 * nb) == all_ok
        wdt = timed(wstep, a.steps)
        wire = {"value": world * nb * a.steps / wdt, "unit": "verifications/s", "ms_per_step": wdt / a.steps * 1e3,
                "note": f"from {wl['wire_len']}-byte wire-format proofs + 32-byte compressed commitments: R1CSProof::from_bytes, point "
                        "decompression, transcript replay and verification on the GPU; per-proof accept bits"}

        # ---- secondary: combined batch check (BASELINE configs[1] 'single big MSM': sum_p rho_p * check_p as ONE point per
        # GPU; RCCL all-gather of the 64-byte partials + local add when n_gpus > 1).
        import random
        rnd = random.Random(0xC0B1 + rank)   # verifier-chosen weights: any scalars < 2^250 < n
        d_rho = gpu.to_device(b"".join(rnd.getrandbits(250).to_bytes(32, "little") for _ in range(nb)))
        d_parts = [gpu.malloc(64) for _ in ctxs]

        def cstep(i):
            p_, s_, c_ = batch_ptrs(i + rank_off)
            ctxs[i % len(ctxs)].r1cs_verify_combined_dev(gens, circ, nb, n1, k, p_, s_, c_, d_rho, d_parts[i % len(ctxs)])

        for i in range(len(ctxs)):
            cstep(i)
        sync_all()
        cdt = timed(cstep, a.steps)
        part = ctxs[0].download(d_parts[0], 64)
        if world > 1:
            from mpc_bulletproof_amd import sharding
            part = sharding.combine_partial_points(part, gpu.points_sum)
        assert part == bytes(64), "combined batch check must be the identity for valid proofs"
        comb = {"value": world * nb * a.steps / cdt, "unit": "verifications/s", "ms_per_step": cdt / a.steps * 1e3,
                "vs_per_proof_value": (world * nb * a.steps / cdt) / (world * nb * a.steps / dt),
                "note": "sum_p rho_p*mega_check_p == identity (single accept bit per batch; one fixed-base MSM over the 130 "
                        f"generators + one {nb * (11 + m + 2 * k)}-term bucket-method MSM per GPU; partial points all-gathered "
                        "over RCCL when n_gpus > 1)"}

    # ======== the other half of BASELINE.json's metric: R1CS constraints/s of the PROVER (configs[2]: 256 provers in lock-step, each
    # range-proving 16 x 64-bit values in one constraint system: n = 1024 multipliers, q = 2064 constraints), through the C++ host
    # mirror of the reference API over the C ABI.  A stream of batches on `prover_threads` worker threads, one context each.
    prove = shuffle = None
    steps_in_flight = len(ctxs)
    if a.full and world == 1 and not a.no_prover:
        # the verification legs are done: their contexts (20 streams with hardware queues of their own) go, so that the prover's worker
        # contexts do not share queues with them; ctxs[0] keeps the circuit and the tables alive until the end
        steps_in_flight = len(ctxs)
        for c in ctxs[1:]:
            c.close()
        ctxs = ctxs[:1]
        # (the secondary legs below must not cost a run its headline line: a failure -- incl. a failed correctness assertion on the
        # prover's output -- is reported in the leg's place, loudly on stderr as well)
        try:
            import ctypes as C
            host = C.CDLL(os.path.join(ROOT, "tests", "host", "libbph_capi.so"))
            vals = [((0x9E3779B97F4A7C15 * (i + 1 + 31 * p)) & ((1 << 64) - 1)) for p in range(P_NB) for i in range(P_NVALS)]
            arr = (C.c_uint64 * len(vals))(*vals)
            lab = (C.c_uint8 * len(LABEL)).from_buffer_copy(LABEL)
            OS_ENTROPY = (1 << 64) - 1

            def stream(nbatch, threads, prebuild, profile):
                pout, plen_ = (C.c_uint8 * (nbatch * P_NB * 4096))(), C.c_size_t(0)
                pcom, ms_ = (C.c_uint8 * (nbatch * P_NB * P_NVALS * 64))(), (C.c_double * 12)()
                rc = host.bph_range_prove_stream(C.c_size_t(nbatch), C.c_size_t(threads), C.c_int(prebuild), C.c_int(profile), C.c_size_t(P_NB),
                                                 C.c_size_t(P_NVALS), C.c_size_t(N_BITS), lab, C.c_size_t(len(LABEL)), arr, C.c_uint64(OS_ENTROPY),
                                                 C.c_size_t(P_N), pout, C.byref(plen_), pcom, ms_)
                assert rc == 0, f"bph_range_prove_stream rc={rc}"
                return list(ms_), pout, plen_.value, pcom

            T, NBAT = max(1, a.prover_threads), max(1, a.prover_batches)
            stream(2, 1, 1, 0)            # generator tables (20 GB, c = 14), workspaces, pools, the cached circuit
            stream(2 * T, T, 1, 0)        # every worker's context warm
            best = None
            for rep in range(3):
                r = stream(NBAT, T, 1, 0)
                if best is None or r[0][0] < best[0][0]:
                    best = r
            ms_b, pout, plen_v, pcom = best
            # a sample of the proofs made inside the timed region must verify: GPU verifier here, the CPU oracle in the fork pool
            param = N_BITS | (P_NVALS << 16)
            sample = [(bi, p) for bi in sorted({0, NBAT // 2, NBAT - 1}) for p in (0, 101, P_NB - 1)]
            pb, cb = bytes(pout), bytes(pcom)
            chk = []
            for bi, p in sample:
                i = bi * P_NB + p
                proof_i, com_i = pb[i * plen_v:(i + 1) * plen_v], cb[i * P_NVALS * 64:(i + 1) * P_NVALS * 64]
                mega = (C.c_uint8 * 64)()
                vv = (C.c_uint64 * 1)()
                rc = host.bph_r1cs_verify(4, C.c_size_t(param), lab, C.c_size_t(len(LABEL)), vv, C.c_size_t(0),
                                          (C.c_uint8 * len(com_i)).from_buffer_copy(com_i), C.c_size_t(P_NVALS),
                                          (C.c_uint8 * len(proof_i)).from_buffer_copy(proof_i), C.c_size_t(len(proof_i)), C.c_size_t(P_N), mega)
                assert rc == 0, f"a proof of the timed prover stream does not verify (batch {bi}, prover {p}): rc={rc}"
                chk.append((4, param, LABEL, com_i, proof_i, P_N))
            oracle_checked = 0
            if pool is not None:
                verdicts = pool.map(_cpu_check_proofs, [chk[:2], chk[-2:]])
                assert all(v == 0 for vs in verdicts for v in vs), "the CPU oracle rejects a proof of the timed prover stream"
                oracle_checked = 4
            assert len({pb[i * plen_v:(i + 1) * plen_v] for i in range(NBAT * P_NB)}) == NBAT * P_NB      # every proof is a different one
            # the same stream with HIP-event timing of the device phases (separate region): GPU-busy share, the dominant kernel's residency;
            # one worker alone: the dominant kernel's SOLO duration; circuit building inside the timed region
            ms_p = stream(NBAT, T, 1, 1)[0]
            nsolo = max(2, NBAT // 4)
            ms_s = stream(nsolo, 1, 1, 1)[0]
            ms_full = min((stream(NBAT, T, 0, 0)[0] for _ in range(2)), key=lambda r: r[0])
            wall = ms_b[0]
            per_launch_bytes = 2 * P_NB * (1 + P_N) * 96          # 512 L / R MSMs of 1 + n terms, 96 B per term
            solo_msm_ms = ms_s[5] / max(ms_s[6], 1)
            pmc_p = None
            if os.path.exists(PMC_FILE):
                with open(PMC_FILE) as f:
                    pmc_p = json.load(f).get("prover")
            prove = {"value": NBAT * P_NB * P_Q / wall * 1e3, "unit": "R1CS constraints/s", "proofs_per_s": NBAT * P_NB / wall * 1e3,
                     "ms_per_batch": wall / NBAT,
                     "workload": f"{NBAT} batches x {P_NB} provers x ({P_NVALS} x 64-bit range gadgets in one constraint system: n = {P_N}, q = {P_Q}, m = {P_NVALS}), "
                                 f"{T} worker threads with a context each",
                     "timed": "Prover::prove_batch for every batch incl. dropping the provers (Prover::prove consumes self): the reference's own bench "
                              "times proof generation only, with the constraint system built beforehand (benches/r1cs.rs:36-55, 95-108).  Blinding factors "
                              "from the default RNG (OsRng; the blinding vectors s_L, s_R are expanded on the device from one key per prover).  Best of 3 streams",
                     "proofs_checked": {"gpu_verifier": len(sample), "cpu_oracle": oracle_checked, "distinct_proofs": NBAT * P_NB},
                     "host_ms_per_batch": {"prove_batch": ms_b[2] / NBAT, "drop": ms_b[3] / NBAT, "circuit_building_untimed": ms_b[1] / NBAT},
                     "incl_circuit_building": {"value": NBAT * P_NB * P_Q / ms_full[0] * 1e3, "unit": "R1CS constraints/s", "ms_per_batch": ms_full[0] / NBAT,
                                               "note": "the same stream with gadget building (256 x 2064 constraint rows), the 4096 Pedersen commitments and the "
                                                       "provers' set-up inside the timed region as well"},
                     "single_thread": {"value": P_NB * P_Q / (ms_s[0] / nsolo) * 1e3, "unit": "R1CS constraints/s",
                                       "ms_per_batch": ms_s[0] / nsolo, "note": "one worker thread, batches back to back (with event timing on)"},
                     "roofline": {"bound": "hbm", "kernel": "k_fixed_msm_ipp<16,128> (+ its block sum): the L / R table-lookup MSMs of one IPP round, 512 MSMs of 1025 terms",
                                  "achieved": per_launch_bytes / (solo_msm_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": per_launch_bytes / (solo_msm_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": (pmc_p or {}).get("traffic_bytes_round_msm"),
                                  "avg_launch_ms": solo_msm_ms, "launches": int(ms_s[6]), "algorithmic_bytes_per_launch": per_launch_bytes,
                                  "timed": "HIP-event pairs on the launch stream around the kernel, one worker thread (no other batch on the GPU)",
                                  "residency_in_the_stream_ms": ms_p[5] / max(ms_p[6], 1),
                                  "note": "VALU-integer bound like every kernel here: 16 table additions (~1 650 instructions each) per 96 algorithmic bytes; the binding roofline is roofline_valu_issue beside this one"},
                     "gpu_busy": {"frac": ms_p[4] / ms_p[0], "busy_ms_per_batch": ms_p[4] / NBAT, "wall_ms_per_batch": ms_p[0] / NBAT,
                                  "device_phase_ms_per_batch": {"ipp_rounds": ms_p[7] / NBAT, "phase_commitments": ms_p[8] / NBAT, "polynomials": ms_p[9] / NBAT,
                                                                "T_commitments": ms_p[10] / NBAT, "ipp_setup": ms_p[11] / NBAT},
                                  "what": "union over the worker contexts of the device-phase intervals (HIP events, first to last launch of every call) / wall "
                                          "clock of the stream, measured in a separate stream with event timing on"},
                     "roofline_valu_issue": ({"bound": "VALU issue slots (mix-weighted)", "achieved": pmc_p["valu_wave_instr_per_batch"] / (wall / NBAT * 1e-3),
                                              "peak": VALU_ISSUE_PEAK_MIX, "unit": "wave-instr/s",
                                              "frac": pmc_p["valu_wave_instr_per_batch"] / (wall / NBAT * 1e-3) / VALU_ISSUE_PEAK_MIX,
                                              "valu_wave_instr_per_batch": pmc_p["valu_wave_instr_per_batch"], "source": pmc_p.get("source")} if pmc_p else None),
                     "cpu_baseline": cpu_prove}

            # ---- configs[3] on ONE GPU: the k-shuffle gadget at k = 2^14 (q = 65 533 constraints, n = 32 766 multipliers, all
            # second-phase; m = 32 768 commitments; 98 347-term mega_check): one proof, prove then verify, wall clock of
            # Prover::prove / Verifier::verify with the circuit built beforehand (as the reference's benches/shuffle.rs times them)
            if not os.environ.get("BPGPU_BENCH_NO_SHUFFLE"):
                ks = 1 << 14
                rnd = __import__("random").Random(77)
                xs = [rnd.getrandbits(64) for _ in range(ks)]
                ys = list(xs)
                rnd.shuffle(ys)
                sarr = (C.c_uint64 * (2 * ks))(*(xs + ys))
                sproof, splen, scom, sms = (C.c_uint8 * 8192)(), C.c_size_t(0), (C.c_uint8 * (2 * ks * 64))(), (C.c_double * 6)()
                runs = []
                for rep in range(4):
                    rc = host.bph_shuffle_prove_verify(C.c_size_t(ks), sarr, C.c_uint64(OS_ENTROPY), C.c_size_t(1 << 15), sproof, C.byref(splen), scom, sms)
                    assert rc == 0, f"bph_shuffle_prove_verify rc={rc}"          # rc == 0: the proof was accepted by the GPU verifier
                    if rep:
                        runs.append(list(sms))
                med = [sorted(r[i] for r in runs)[1] for i in range(6)]
                qs = 4 * (ks - 1) + 1
                # the same proof verified against a ParametricCircuit (the gadget's rows affine in its challenge, uploaded once)
                pms = (C.c_double * 3)()
                build_ms = None
                for rep in range(2):
                    rc = host.bph_shuffle_verify_param(C.c_size_t(ks), scom, sproof, C.c_size_t(splen.value), C.c_size_t(1 << 15), C.c_size_t(5), pms)
                    assert rc == 0, f"bph_shuffle_verify_param rc={rc}"
                    if rep == 0:
                        build_ms = pms[0]
                # ... and the prover bound to the same circuit (Prover::use_circuit: the gadget runs for its witness only)
                ppms = (C.c_double * 3)()
                pruns = []
                pproof, pplen, pcom = (C.c_uint8 * 8192)(), C.c_size_t(0), (C.c_uint8 * (2 * ks * 64))()
                for rep in range(4):
                    rc = host.bph_shuffle_prove_param(C.c_size_t(ks), sarr, C.c_uint64(OS_ENTROPY), C.c_size_t(1 << 15), pproof, C.byref(pplen), pcom, ppms)
                    assert rc == 0, f"bph_shuffle_prove_param rc={rc}"
                    assert host.bph_shuffle_verify_param(C.c_size_t(ks), pcom, pproof, C.c_size_t(pplen.value), C.c_size_t(1 << 15), C.c_size_t(1), pms) == 0
                    if rep:
                        pruns.append(list(ppms))
                pmed = [sorted(r[i] for r in pruns)[1] for i in range(3)]
                shuffle = {"workload": f"k-shuffle gadget, k = 2^14: q = {qs} constraints, n = {2 * (ks - 1)} multipliers (phase 2), m = {2 * ks}, padded n = 2^15",
                           "prove": {"value": qs / med[3] * 1e3, "unit": "R1CS constraints/s", "ms": med[3], "best_ms": min(r[3] for r in runs),
                                     "circuit_building_ms": med[2]},
                           "verify": {"value": qs / med[5] * 1e3, "unit": "R1CS constraints/s", "ms": med[5], "best_ms": min(r[5] for r in runs),
                                      "circuit_building_ms": med[4]},
                           "prove_parametric_circuit": {"value": qs / pmed[2] * 1e3, "unit": "R1CS constraints/s", "ms": pmed[2], "circuit_building_ms": pmed[1],
                                                        "note": "Prover::prove with the prover bound to the ParametricCircuit (Prover::use_circuit): the gadget runs for its "
                                                                "witness only, no constraint rows are built, hashed or uploaded (bpgpu_r1cs_prover_session_polys_param); "
                                                                "every proof verified against the same circuit; median of 3"},
                           "verify_parametric_circuit": {"value": qs / pms[2] * 1e3, "unit": "R1CS constraints/s", "ms": pms[2], "commit_calls_ms": pms[1],
                                                         "circuit_capture_ms_once_per_shape": build_ms,
                                                         "note": "Verifier::verify(proof, gens, ParametricCircuit): the gadget's 65 533 rows cross the ABI once per circuit "
                                                                 "shape (bpgpu_circuit_create_param: coefficients c0 + chi c1), a verification = transcript replay + one "
                                                                 "bpgpu_r1cs_verify_batch_param call; median of 5"},
                           "note": "one proof on one GPU, medians (and best) of 3; every proof verified (the call fails otherwise); OsRng blinding "
                                   "factors.  A third of prove and half of verify is the host mirror running the gadget (65 533 constraint rows "
                                   "carrying the challenge): these two figures move with whatever else the box's CPUs are doing; circuit_building = "
                                   "the 32 768 commit calls before prove / verify (a dependent hash chain on the host)"}
        except Exception as e:      # noqa: BLE001
            import traceback
            traceback.print_exc()
            failed = {"error": f"{type(e).__name__}: {e}"}
            prove = prove or failed
            shuffle = shuffle or failed

    # ======== N > 1: configs[3] in its sharded form -- ONE 2^14-shuffle proof split over the ranks (every multi-scalar multiplication
    # by generator / point range, partial points all-gathered over RCCL and added: SURVEY 8e.2), proved and verified on all of them
    shuffle_sharded = None
    if a.full and world > 1 and not a.no_prover and not os.environ.get("BPGPU_BENCH_NO_SHUFFLE"):
        import ctypes as C
        from mpc_bulletproof_amd import sharding
        host = C.CDLL(os.path.join(ROOT, "tests", "host", "libbph_capi.so"))
        host.bph_set_device(C.c_int(dev))
        cb = sharding.allgather_callback()
        ks = 1 << 14
        rnd = __import__("random").Random(77)
        xs = [rnd.getrandbits(64) for _ in range(ks)]
        ys = list(xs)
        rnd.shuffle(ys)
        sarr = (C.c_uint64 * (2 * ks))(*(xs + ys))
        sproof, splen, scom, sms = (C.c_uint8 * 8192)(), C.c_size_t(0), (C.c_uint8 * (2 * ks * 64))(), (C.c_double * 6)()
        runs, runs_p = [], []
        err = None
        for fn_name, dst in (("bph_shuffle_prove_verify_sharded", runs), ("bph_shuffle_prove_verify_sharded_param", runs_p)):
            for rep in range(4):
                fence()
                rc = getattr(host, fn_name)(C.c_size_t(ks), sarr, C.c_uint64((1 << 64) - 1), C.c_size_t(1 << 15), C.c_size_t(rank), C.c_size_t(world),
                                            cb, None, sproof, C.byref(splen), scom, sms)
                # a failure of this secondary leg (every rank sees the same return code: they compute the same proof) must not cost the
                # run its headline line: it is reported in place of the figures
                if sharding.max_over_ranks(float(rc != 0)) != 0:
                    err = f"{fn_name} returned {rc} on rank {rank} (repetition {rep})"
                    break
                if rep:
                    dst.append([sharding.max_over_ranks(x) for x in sms])
            if err:
                break
        qs = 4 * (ks - 1) + 1
        if err:
            shuffle_sharded = {"ranks": world, "error": err}
        else:
            med = [sorted(r[i] for r in runs)[1] for i in range(6)]
            medp = [sorted(r[i] for r in runs_p)[1] for i in range(6)]
            shuffle_sharded = {"ranks": world, "workload": f"ONE k-shuffle proof, k = 2^14 (q = {qs} constraints, 2^15 generators per side, a 98 347-term mega_check), "
                                                           "split over the ranks by generator / point range",
                               "prove": {"value": qs / med[3] * 1e3, "unit": "R1CS constraints/s", "ms": med[3]},
                               "verify": {"value": qs / med[5] * 1e3, "unit": "R1CS constraints/s", "ms": med[5]},
                               "parametric_circuit": {"prove_ms": medp[3], "verify_ms": medp[5],
                                                      "note": "prover and verifier of every rank bound to the shuffle's ParametricCircuit (no constraint rows built or uploaded per proof)"},
                               "note": "max over ranks, medians of 3; latency-bound: 15 IPP rounds, each with an all-gather of two 64-byte partial points and a host hash"}

    if pool is not None:
        pool.close()
        pool.join()

    if rank == 0:
        nvar = 11 + m + 2 * k
        nterms = 13 + m + 2 * (1 << k) + 2 * k
        W = 252 // a.window_bits + 1
        # The kernels of the window-parallel chain that consume algorithmic bytes (96 B per MSM term = 64 B point +
        # 32 B scalar) and what each reads of them; the dominant kernel = the one with the longest solo duration.
        lpm = 16 if nb >= 1024 else 32
        # (from 256 proofs on the generator half of the back launch is walked a proof per lane: k_verify_back_q, csrc/fixed_body.cuh)
        names = {"verify_back": f"k_verify_back_q<{a.window_bits},1>" if nb >= 256 else f"k_verify_back<{a.window_bits},{lpm}>", "verify_front": "k_verify_front<4>",
                 "verify_windows": "k_verify_windows", "verify_scalars": "k_verify_scalars_fast", "verify_groups": "k_verify_horner_groups",
                 "verify_verdict": "k_verify_verdict"}
        bytes_per_proof = {"verify_back": (nterms - nvar) * 96, "verify_front": nvar * 64, "verify_windows": nvar * 32,
                           "verify_scalars": (6 + k + 5) * 32 + nterms * 32}
        pmc = None
        if os.path.exists(PMC_FILE):
            with open(PMC_FILE) as f:
                pmc = json.load(f)
        lib_hash = _lib_hash()
        # the counters belong to ONE binary: instructions per step counted on another build of libbpgpu.so are reported as stale, not as a roofline
        pmc_ok = bool(pmc) and nb == 1024 and a.window_bits == 20 and pmc.get("lib_sha256_16") == lib_hash
        pmc_stale = ({"measured_on_lib_sha256_16": pmc.get("lib_sha256_16"), "this_lib_sha256_16": lib_hash,
                      "valu_wave_instr_per_step_1024": pmc.get("valu_wave_instr_per_step_1024"),
                      "note": "profiles/pmc_constants.json was counted on a different libbpgpu.so: no VALU roofline is computed from it (tools/pmc_constants.py regenerates it)"}
                     if pmc and not pmc_ok and nb == 1024 and a.window_bits == 20 else None)
        roof = per_kernel = None
        step_s = dt / a.steps
        if solo:
            cand = [n_ for n_ in bytes_per_proof if n_ in solo]
            dom = max(cand, key=lambda n_: solo[n_][0])
            solo_ms, solo_cnt = solo[dom]
            alg_bytes = nb * bytes_per_proof[dom]
            achieved = alg_bytes / (solo_ms * 1e-3) / 1e9
            traffic = (pmc or {}).get("traffic_bytes_per_launch", {}).get(dom)
            res_step = replay["resident_ms_per_step"].get(dom)
            step_bytes = nb * (nterms * 96 + (6 + k + 5) * 32)
            pmc_fresh = bool(pmc) and pmc.get("lib_sha256_16") == lib_hash
            res_ms = res_step if res_step else solo_ms
            ach_x = alg_bytes / (res_ms * 1e-3) / 1e9
            roof = {"bound": "hbm", "kernel": names[dom], "achieved": ach_x, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": ach_x / HBM_PEAK_GBS, "traffic": (traffic if pmc_fresh else None), "avg_launch_ms": res_ms,
                    "algorithmic_bytes_per_launch": alg_bytes, "launches": replay["launches"].get(dom),
                    "timed": "HIP-event pairs on the launch streams around EVERY launch of this kernel in a replay of the timed steps on all "
                             "contexts; the duration is the UNION of its launch intervals / steps = the share of a step's wall clock during which "
                             "the kernel is on the chip.  Exclusive by construction: it cannot exceed the replay's ms_per_step "
                             f"({replay['ms_per_step']:.4f} ms; the timed region's: {step_s * 1e3:.4f} ms)",
                    "solo": {"avg_launch_ms": solo_ms, "launches": solo_cnt, "achieved": achieved, "frac": achieved / HBM_PEAK_GBS,
                             "what": "the same kernel in un-pipelined steps on one context (what `rocprofv3 --kernel-trace` of a solo run measures, "
                                     "pmc_constants.json solo_us): the LATENCY of a launch that occupies a third of the SIMDs -- several such "
                                     "launches are co-resident in the timed run, so this duration exceeds ms_per_step and is NOT the roofline input",
                             "solo_reference_us": ((pmc or {}).get("solo_us", {}).get(dom) if pmc_fresh else None)},
                    "whole_step": {"algorithmic_bytes": step_bytes, "achieved": step_bytes / step_s / 1e9, "frac": step_bytes / step_s / 1e9 / HBM_PEAK_GBS,
                                   "what": "all algorithmic bytes of a step / the timed region's ms_per_step"},
                    "traffic_stale": (None if pmc_fresh or not traffic else {"bytes": traffic, "measured_on_lib_sha256_16": (pmc or {}).get("lib_sha256_16")}),
                    "valu_issue_frac": None,
                    "note": "The path is VALU-integer bound, not HBM bound: 252-bit modular arithmetic spends ~1 650 instructions per 96 "
                            "algorithmic bytes (valu_issue_frac here = roofline_valu_issue.frac, the binding roofline).  `traffic` (PMC, per launch, "
                            "FETCH_SIZE / WRITE_SIZE as MI355X_MICROARCH.md prescribes, counted on a run over DISTINCT batches) exceeds the algorithmic "
                            "bytes because every term gathers 13 random 64-byte rows of the 57 GB fixed-base table (each a 128-byte line) -- bytes spent to delete doublings"}
            if pmc_ok:
                # per kernel: VALU wave-instructions (rocprofv3 --pmc SQ_INSTS_VALU, solo) / its solo duration measured HERE / the issue
                # peak of the SIMDs its waves occupy (waves < 1024: one SIMD each)
                per_kernel = {}
                for n_, full in names.items():
                    if n_ in solo and n_ in pmc.get("valu_wave_instr_per_launch", {}):
                        instr, waves = pmc["valu_wave_instr_per_launch"][n_], (pmc.get("waves_per_launch") or {}).get(n_)
                        simds = min(N_SIMD, int(waves)) if waves else N_SIMD
                        per_kernel[full] = {"valu_wave_instr": instr, "solo_ms": solo[n_][0], "waves": waves, "simds_occupied": simds,
                                            "frac_of_occupied_simds_issue_peak": instr / (solo[n_][0] * 1e-3) / (simds * SIMD_ISSUE_PEAK_MIX),
                                            "frac_of_chip_issue_peak": instr / (solo[n_][0] * 1e-3) / VALU_ISSUE_PEAK_MIX}
        # integer roofline: algorithmic F_p multiplications x 94 limb MADs each (csrc/fe29.cuh), per step.  Per non-identity proof
        # point 7 table additions + 60 window additions (mixed, 11 mul), one inversion per 4 points (~310), per proof 252
        # doublings (9) + 64 additions (16) in the Horner passes; fixed-base: one mixed addition per (generator, window) + the
        # 16-lane butterfly.  A_I2, A_O2, S2 are the identity in 1-phase proofs and are skipped.
        fp_var = nb * ((nvar - 3) * (7 + 60) * 11 + ((nvar + 3) // 4) * 310 + 252 * 9 + 64 * 16)
        fp_fixed = nb * ((nterms - nvar) * W * 11 + 15 * 16)
        valu = None
        if pmc_ok:
            instr = pmc["valu_wave_instr_per_step_1024"]
            valu = {"bound": "VALU issue slots (mix-weighted)", "achieved": instr / step_s, "peak": VALU_ISSUE_PEAK_MIX,
                    "unit": "wave-instr/s", "frac": instr / step_s / VALU_ISSUE_PEAK_MIX,
                    "valu_wave_instr_per_step": instr, "measured_on_lib_sha256_16": pmc.get("lib_sha256_16"),
                    "this_lib_sha256_16": lib_hash, "binary_matches": pmc.get("lib_sha256_16") == lib_hash,
                    "per_kernel_solo": per_kernel,
                    "flat_4_cycle_frac": instr / step_s / (N_SIMD * 2.4e9 / 4.0),
                    "note": "The binding roofline of this path.  instructions per step: rocprofv3 --pmc SQ_INSTS_VALU of a solo run (" + pmc.get("source", "profiles/") +
                            "); peak = 1024 SIMDs x 2.4 GHz / 4.25 cycles per wave64 instruction.  The 4.25 is a v_mad_i64_i32-MIX figure, self-measured: "
                            "the issue rate of THIS instruction mix (74 % v_mad_i64_i32, a quarter-rate 64-bit multiply-add) in the doubling / addition "
                            "micro-benchmarks at 8 waves/SIMD (profiles/r01_microbench_primitives.log); the guide prices plain wave64 VALU at 2 cycles "
                            "with >= 2 waves/SIMD, which no kernel of this mix can reach.  flat_4_cycle_frac: against one instruction per 4 cycles.  "
                            "per_kernel_solo: each kernel alone, against the SIMDs its waves occupy.  The peak is priced at 2.4 GHz; a sustained "
                            "run of this path draws the board's 1.36 kW and is held at 2.30 GHz (profiles/r04_power_phases.log), so at the clock "
                            "actually held a long run's frac is 4 % higher than printed"}
            if roof:
                roof["valu_issue_frac"] = valu["frac"]
        out = {
            "metric": "range-proof verifications/sec (64-bit, m=1)",
            "value": world * nb * a.steps / dt, "unit": "verifications/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u32x9 (29-bit limbs, 252-bit prime fields)", "data": "synthetic",
            "config": {"workload": f"batch verify {nb} x 64-bit range-gadget R1CS proofs (m=1, n=64, 154-term "
                                   f"mega_check MSM per proof, per-proof accept bits) per GPU; every step verifies a different batch "
                                   f"({nbat} distinct batches = {nbat * nb} different proofs, cycled)",
                       "distinct_batches": nbat,
                       "untimed_lead_in": (f"{int(os.environ.get('BPGPU_WARM_BURSTS', '8'))} repetitions of the timed region's own pattern ({a.steps} steps, then a "
                                           "synchronisation) after the continuous warm-up: a short run is a burst, and the clocks settle on the load pattern "
                                           "(profiles/r04_burst_precondition.log)" if a.steps <= 256 and int(os.environ.get('BPGPU_WARM_BURSTS', '8')) else
                                           "one un-timed step per context right up to the opening fence, after the continuous warm-up"),
                       "value_replaying_one_batch": (world * nb * a.steps / dt_same if dt_same else None),
                       "second_metric": ({"name": "R1CS constraints/s of the prover (configs[2]: 256 provers x (16 x 64 bit))", "value": prove.get("value"),
                                          "unit": "R1CS constraints/s", "cpu_baseline": (cpu_prove or {}).get("value")} if prove else None),
                       "h2d_inclusive_value": (h2d or {}).get("value"),
                       "window_bits": a.window_bits, "proofs_per_step_per_gpu": nb, "steps_in_flight": steps_in_flight,
                       "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
                       "untimed_before_the_timed_region": f"max(warmup, steps_in_flight) steps, result check, {warm_s:.1f} s of further untimed "
                                                          "steps (clocks), one hand-over step per context"},
            "roofline": roof,
            "roofline_valu_issue": valu,
            "roofline_valu_issue_stale": pmc_stale,
            "value_replaying_one_batch": ({"value": world * nb * a.steps / dt_same, "unit": "verifications/s", "ms_per_step": dt_same / a.steps * 1e3,
                                           "note": "the same timed region verifying ONE batch over and over (rounds 1-3's figure): its 110 MB of fixed-base "
                                                   "table rows stay in the 256 MiB Infinity Cache; `value` cycles through distinct batches"}
                                          if dt_same else None),
            "r1cs_constraints_per_s": (prove or {}).get("value"),
            "roofline_int": {"bound": "valu_int (v_mad_u64_u32)", "scope": "variable-base + fixed-base halves of one step's mega_check MSMs / wall time per step",
                             "achieved": (fp_var + fp_fixed) * 94 / step_s / 1e12, "peak": MAD_PEAK_TOPS, "unit": "Tmad/s",
                             "frac": (fp_var + fp_fixed) * 94 / step_s / 1e12 / MAD_PEAK_TOPS},
            "kernel_solo_ms": ({n_: v[0] for n_, v in solo.items()} if solo else None),
            "pipelined_replay": replay,
            "cpu_baseline": cpu,
            "cpu_baseline_1t": cpu1,
            "h2d_inclusive": h2d,
            "one_call": one_call,
            "single_batch": single,
            "with_device_transcript": fs,
            "from_wire_format": wire,
            "combined_batch_check": comb,
            "r1cs_prove": prove,
            "shuffle_2e14": shuffle,
            "shuffle_2e14_sharded": shuffle_sharded,
            "range_prove": ({"value": nb / wl["prove_seconds"], "unit": "64-bit range proofs/s", "ms_per_batch": wl["prove_seconds"] * 1e3,
                             "note": f"the {nb} proofs of this workload, proved in lock-step by the GPU prover while it was generated "
                                     "(wall clock incl. host circuit building and transcripts)"} if wl.get("prove_seconds") else None),
        }
        out["full"] = a.full
        if cpu is None:
            out["cpu_baseline_reason"] = "--no-cpu-baseline" if a.full else "measured with --full only"
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    gpu.gens_destroy(gens)
    gpu.circuit_destroy(circ)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
