#!/usr/bin/env python3
"""The two-call prover of two-phase circuits (bpgpu_r1cs_prove_fs2_begin / _finish) against the staged sequence, on the k-shuffle
(tests/r1cs.rs:23-62: no phase-1 multipliers, n = 2 (k - 1) in phase 2, m = 2k).  Writes profiles/prove_fs2.log (the source of the
figures in DESIGN.md):

  dev     bpgpu_r1cs_prove_fs2_begin_dev + _finish_dev back to back on resident operands, HIP events on the context's stream around
          the pair: what the GPU spends on a batch when the host neither hashes nor waits (vector-key blindings; the phase-2 witness
          is the gadget's under the model's challenge -- the time does not depend on its values).  256 x 8-shuffle, 16 x 2^10-shuffle;
  mirror  Prover::prove of the host mirror with the prover bound to the shuffle's ParametricCircuit, wall clock, k = 2^10 and 2^14:
          the staged route and the fused one (BPH_PROVE_FUSED=1, read per call) alternate in ONE process; ratio = staged / fused.

WARM untimed steps, then STEPS timed ones per route, medians (min..max) in ms.  Both routes produce the same proof bytes under a
seeded Rng (asserted)."""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

WARM, STEPS = 3, 20
LABEL = b"shuffle challenge"


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):8.3f}..{max(ts):9.3f})"


def mirror(ks):
    """wall clock of Prover::prove through the harness on both routes, alternating"""
    host = C.CDLL(os.path.join(ROOT, "tests", "host", "libbph_capi.so"))
    xs = [((0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1)) for i in range(ks)]
    arr = (C.c_uint64 * (2 * ks))(*(xs + xs[1:] + xs[:1]))
    cap = max(2, 2 * ks)
    proof, plen, com, ms3 = (C.c_uint8 * 8192)(), C.c_size_t(0), (C.c_uint8 * (2 * ks * 64))(), (C.c_double * 3)()
    ts, last = {"staged": [], "fused": []}, {}
    for step in range(WARM + STEPS):
        for route in ("staged", "fused"):
            if route == "fused":
                os.environ["BPH_PROVE_FUSED"] = "1"
            else:
                os.environ.pop("BPH_PROVE_FUSED", None)
            rc = host.bph_shuffle_prove_param(C.c_size_t(ks), arr, C.c_uint64(901), C.c_size_t(cap), proof, C.byref(plen), com, ms3)
            assert rc == 0, rc
            if step >= WARM:
                ts[route].append(ms3[2])                      # Prover::prove alone (the commitments and the gadget are the same work)
            last[route] = bytes(proof)[:plen.value]
    assert last["staged"] == last["fused"], "the fused and the staged route disagree on the proof bytes"
    return ts


def device(nb, ks):
    """HIP-event time of the two _dev calls on resident operands"""
    import random
    import mpc_dealer as md
    import oracle_lib as o
    import pymodel as pm
    import mpc_bulletproof_amd as m
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    n, mm = 2 * (ks - 1), 2 * ks
    # the parametric circuit and one prover's phase-2 witness from the model's gadget; every prover of the batch takes that witness
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"ShuffleProofTest"))
    pv.pc_gens.commit = lambda v, b: pm.G           # the commitments play no part here: skip the model's scalar multiplications
    xs = [((0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1)) for i in range(ks)]
    vars_ = [pv.commit(v, 1)[1] for v in xs + xs[1:] + xs[:1]]
    pm.shuffle_gadget(pv, vars_[:ks], vars_[ks:])
    pv._create_randomized_constraints()
    assert len(pv.a_L) == n
    rp, kd, ix, cf, _ = md.circuit_rows(pv.constraints, param=True)
    rnd = random.Random(nb)
    rb = lambda cnt: bytes(rnd.getrandbits(8) for _ in range(cnt))      # noqa: E731
    wit = lambda v: b"".join(md.mont(x) for x in v) * nb               # noqa: E731
    scal = lambda cnt: b"".join(md.mont(rnd.randrange(pm.N)) for _ in range(cnt))      # noqa: E731
    k = (n - 1).bit_length()
    gpu = m.BpGpu(0)
    gens = gpu.gens_create(o.gens("G", 1 << k), o.gens("H", 1 << k), o.generator(), o.generator(), 8)
    circ = gpu.circuit_create_param(len(pv.constraints), 1, rp, kd, ix, cf, n, mm)
    ins = [gpu.to_device(x) for x in (rb(32 * nb), scal(nb * 3), wit(pv.a_L), wit(pv.a_R), wit(pv.a_O), rb(32 * nb), scal(nb * mm), scal(nb * 8))]
    outs = [gpu.malloc(s) for s in (64 * nb * (11 + 2 * k), 160 * nb)]
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    st = C.c_void_p(gpu.stream())
    ts = []
    for step in range(WARM + STEPS):
        assert hip.hipEventRecord(ev[0], st) == 0
        sess = gpu.r1cs_prove_fs2_begin_dev(gens, circ, nb, 0, ins[0], LABEL, ins[1])
        gpu.r1cs_prove_fs2_finish_dev(gens, circ, sess, ins[2], ins[3], ins[4], ins[7], outs[0], outs[1], d_v_blinding=ins[6],
                                      d_vector_keys=ins[5])
        assert hip.hipEventRecord(ev[1], st) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        if step >= WARM:
            ts.append(ms.value)
    assert gpu.input_flag() == 0
    for p in ins + outs:
        gpu.free(p)
    gpu.circuit_destroy(circ)
    gpu.gens_destroy(gens)
    gpu.close()
    return ts


def child(what, a, b):
    if what == "dev":
        print("RESULT", fmt(device(a, b)))
    else:
        ts = mirror(a)
        s, f = statistics.median(ts["staged"]), statistics.median(ts["fused"])
        print("RESULT", f"{fmt(ts['staged'])}   {fmt(ts['fused'])}   {s / f:8.2f}")


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    lines = [f"# tools/bench_prove_fs2.py   k-shuffle provers (n = 2 (k - 1), m = 2k); a fresh process per line, {WARM} warm-up + {STEPS} timed "
             "steps per route: median (min..max) ms",
             "# dev: begin_dev + finish_dev back to back, HIP events"]

    def run(*args):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], capture_output=True, text=True,
                             timeout=900)
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
        assert out.returncode == 0 and got, (args, out.stdout[-2000:], out.stderr[-2000:])
        return got[0][len("RESULT "):]
    for nb, ks in ((256, 8), (16, 1 << 10)):
        lines.append(f"dev     nb = {nb:<4d} k = {ks:<6d} {run('dev', nb, ks)}")
        print(lines[-1])
        sys.stdout.flush()
    lines.append("# mirror: Prover::prove bound to the ParametricCircuit, wall clock, the two routes alternating in one process")
    lines.append("#                            staged                                fused (BPH_PROVE_FUSED=1)            staged/fused")
    for ks in (1 << 10, 1 << 14):
        lines.append(f"mirror  nb = 1    k = {ks:<6d} {run('mirror', ks, 0)}")
        print(lines[-1])
        sys.stdout.flush()
    path = os.path.join(ROOT, "profiles", "prove_fs2.log")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
