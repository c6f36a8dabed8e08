#!/usr/bin/env python3
"""The pool (bpgpu_pool_r1cs_verify_stream) beside a plain context (bpgpu_r1cs_verify_stream) on the 64-bit range workload: the rate
of one call over --proofs proofs through a plain context, through pools of 1, 2, .. bpgpu_device_count() DISTINCT devices, and
through the list [0, 0] (two slots on one device).  Nothing is gated on these numbers: they say what the pool costs on top of a
context (the pool-of-one / plain ratio) and, on a node with several GPUs, how the rate grows with the devices.  On a machine with
ONE GPU the [0, 0] line is a REHEARSAL -- two slots share the device that one context already fills -- and the log says so.

The workload is bench.py's: 1 024 distinct 64-bit range proofs made by the product path (`bench._gen_workload`, kept in tools/_wl/),
repeated to the queue length.  Operands from page-locked memory (bpgpu_host_alloc: the in-place route where the pool's rule allows
it) and from pageable memory (staged copies); medians of --reps calls after two warm-up calls; every accept bit is asserted.

This process never opens the GPU: every GPU step -- the workload, the device count, each leg -- is a fresh child process under its
own `timeout`, started only after the one before it succeeded.  Writes --log (profiles/pool_verify.log).
Usage: bench_pool.py [--proofs 40960] [--reps 7] [--window-bits 16] [--limit 300] [--log profiles/pool_verify.log]"""
import argparse
import json
import os
import pickle
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CACHE = os.path.join(ROOT, "tools", "_wl", "pool_verify.1024")


def lib_hash():
    import hashlib
    with open(os.path.join(ROOT, "mpc_bulletproof_amd", "libbpgpu.so"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


# ---- the children (each opens the GPU, does one thing, prints one line, exits)
def child_workload():
    import bench
    os.makedirs(os.path.dirname(CACHE), exist_ok=True)
    if not os.path.exists(CACHE):
        bench._gen_workload(CACHE, 1024, 1000, 1)
    print(json.dumps({"workload": os.path.relpath(CACHE, ROOT)}))


def child_count():
    import mpc_bulletproof_amd as m
    print(json.dumps({"devices": m.lib.device_count()}))


def child_leg(leg, proofs, reps, window_bits):
    import mpc_bulletproof_amd as m
    with open(CACHE, "rb") as f:
        wl = pickle.load(f)
    nb0 = len(wl["scalars"]) // 160
    n1, n2, k, mm = wl["dims"]
    mult = (proofs + nb0 - 1) // nb0
    nb = mult * nb0
    ops = [wl["points"] * mult, wl["scalars"] * mult, wl["challenges"] * mult]
    gens = (wl["G"], wl["H"], wl["B"], wl["B"], window_bits)
    if leg == "plain":
        gpu = m.BpGpu(0)
        g, c = gpu.gens_create(*gens), gpu.circuit_create(*wl["csr"], n1 + n2, mm)
        call = lambda p, s, ch: gpu.r1cs_verify_stream(g, c, nb, n1, k, mm, p, s, ch, raw=True)        # noqa: E731
        devices = [0]
    else:
        devices = [int(x) for x in leg.split(",")]
        pool = m.BpPool(devices)
        g, c = pool.gens_create(*gens), pool.circuit_create(*wl["csr"], n1 + n2, mm)
        call = lambda p, s, ch: pool.r1cs_verify_stream(g, c, nb, n1, k, p, s, ch, raw=True)            # noqa: E731
    want = (1).to_bytes(4, "little") * nb
    out = {"leg": leg, "devices": devices, "proofs": nb, "reps": reps, "window_bits": window_bits,
           "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "lib": lib_hash()}
    pinned = [m.lib.host_alloc(len(b), b) for b in ops]
    for name, operands in (("page_locked", pinned), ("pageable", ops)):
        ts = []
        for r in range(reps + 2):
            t0 = time.perf_counter()
            ok = call(*operands)
            ts.append(time.perf_counter() - t0)
            assert ok == want, (leg, name, r)
        med = statistics.median(ts[2:])
        out[name + "_ms"], out[name + "_per_s"] = 1e3 * med, nb / med
    for p in pinned:
        m.lib.host_free(p)
    if leg == "plain":
        gpu.gens_destroy(g)
        gpu.circuit_destroy(c)
        gpu.close()
    else:
        pool.gens_destroy(g)
        pool.circuit_destroy(c)
        pool.close()
    print(json.dumps(out))


# ---- the parent
def step(limit, *args):
    """one child under its own time limit -> the JSON object of its last output line; any failure ends the run"""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.exit(f"step {' '.join(map(str, args))} ended with status {r.returncode}: nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proofs", type=int, default=40960)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-bits", type=int, default=16)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "pool_verify.log"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "workload":
        return child_workload()
    if a.child == "count":
        return child_count()
    if a.child:
        return child_leg(a.child, a.proofs, a.reps, a.window_bits)

    common = ["--proofs", a.proofs, "--reps", a.reps, "--window-bits", a.window_bits]
    step(a.limit, "--child", "workload")
    ndev = step(a.limit, "--child", "count")["devices"]
    legs = ["plain"] + [",".join(str(d) for d in range(n)) for n in range(1, ndev + 1)] + ["0,0"]
    rows = [step(a.limit, "--child", leg, *common) for leg in legs]
    by = {r["leg"]: r for r in rows}
    lines = [f"# bpgpu_pool_r1cs_verify_stream beside bpgpu_r1cs_verify_stream on {ndev} x MI355X: ONE call over {rows[0]['proofs']} 64-bit range proofs",
             f"# (1 024 distinct proofs repeated), generator tables of window {a.window_bits}, default stream options (batches of 1 024 on 20 lanes per",
             f"# context), GPU_MAX_HW_QUEUES={rows[0]['hw_queues']} as the caller exported it; medians of {a.reps} calls after two warm-up calls, wall clock of the",
             "# calling thread; every accept bit asserted.  Each leg is a fresh process under its own `timeout`, started after the one",
             "# before it succeeded.  leg = plain: one context; leg = a device list: a pool with one slot per entry.",
             "# Nothing is gated on these numbers."]
    if ndev < 2:
        lines += ["# ONE GPU in this machine: the leg 0,0 is a REHEARSAL of the pool's control flow -- two slots, two host threads, one device that a",
                  "# single context already fills -- and says nothing about scaling over devices.  No multi-GPU rate has been measured."]
    lines += [json.dumps(r) for r in rows]
    for kind in ("page_locked", "pageable"):
        ratio = {"metric": "pool_of_one_over_plain", "operands": kind, "ratio": by["0"][kind + "_per_s"] / by["plain"][kind + "_per_s"]}
        lines.append(json.dumps(ratio))
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
