#!/usr/bin/env python3
"""The one-call prover (bpgpu_r1cs_prove_fs) against the staged sequence, on the prover of BASELINE.json configs[2]: nb provers in
lock-step, each range-proving 16 values of 64 bits in one constraint system (n = 1024 multipliers, q = 2064 constraints, m = 16),
nb = 256, 1, 16.  Writes profiles/prove_fs.log (the source of the figures in DESIGN.md), one line per shape:

  dev     bpgpu_r1cs_prove_fs_dev on resident operands, HIP events on the context's stream around the call: what the GPU spends on a
          batch when the host neither hashes nor waits (vector-key blindings);
  fused   Prover::prove_batch of the host mirror with BPH_PROVE_FUSED=1, wall clock (packing, upload, the call, download);
  staged  the same call on its default route -- commit, session_polys, msm_gens, ipp_begin, run_fs with the transcript hashed on the
          host's thread pool between them --, wall clock; ratio = staged / fused.

Each shape runs in a fresh process: WARM untimed steps, then STEPS timed ones, medians (min..max) in ms.  The fused and the staged
route produce the same proof bytes (asserted)."""
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
NVALS, NBITS = 16, 64
N_MUL = NVALS * NBITS
LABEL = b"RangeProofTest"


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):8.3f}..{max(ts):9.3f})"


def values(nb):
    return [((0x9E3779B97F4A7C15 * (i + 1 + 31 * p)) & ((1 << 64) - 1)) for p in range(nb) for i in range(NVALS)]


def mirror(nb, fused):
    """wall clock of Prover::prove_batch through the harness, and the proof bytes of the last step"""
    if fused:
        os.environ["BPH_PROVE_FUSED"] = "1"
    else:
        os.environ.pop("BPH_PROVE_FUSED", None)
    import oracle_lib as o
    host = C.CDLL(os.path.join(ROOT, "tests", "host", "libbph_capi.so"))
    arr = (C.c_uint64 * (nb * NVALS))(*values(nb))
    proofs, com, plen = (C.c_uint8 * (nb * 4096))(), (C.c_uint8 * (nb * NVALS * 64))(), C.c_size_t(0)
    ts = []
    for step in range(WARM + STEPS):
        t0 = time.perf_counter()
        rc = host.bph_range_prove_batch(C.c_size_t(nb), C.c_size_t(NVALS), C.c_size_t(NBITS), o._buf(LABEL), C.c_size_t(len(LABEL)), arr,
                                        C.c_uint64(900), C.c_size_t(N_MUL), proofs, C.byref(plen), com)
        assert rc == 0, rc
        if step >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts, bytes(proofs)[:plen.value * nb]


def device(nb):
    """HIP-event time of bpgpu_r1cs_prove_fs_dev on resident operands"""
    import random
    import mpc_dealer as md
    import oracle_lib as o
    import pymodel as pm
    import mpc_bulletproof_amd as m
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    # the circuit and one prover's witness from the model's gadget (16 range gadgets in one constraint system); every prover of
    # the batch takes that witness under blindings of its own
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(LABEL))
    pv.pc_gens.commit = lambda v, b: pm.G           # the commitments play no part here: skip the model's scalar multiplications
    for v in values(1):
        _, var = pv.commit(v, 1)
        pm.range_proof_gadget(pv, pm.lc_var(var), v, NBITS)
    rp, kd, ix, cf, _ = md.circuit_rows(pv.constraints)
    rnd = random.Random(nb)
    rb = lambda k: bytes(rnd.getrandbits(8) for _ in range(k))      # noqa: E731
    wit = lambda v: b"".join(md.mont(x) for x in v) * nb            # noqa: E731
    k = (N_MUL - 1).bit_length()
    gpu = m.BpGpu(0)
    gens = gpu.gens_create(o.gens("G", N_MUL), o.gens("H", N_MUL), o.generator(), o.generator(), 8)
    circ = gpu.circuit_create(rp, kd, ix, cf, N_MUL, NVALS)
    scal = lambda cnt: b"".join(md.mont(rnd.randrange(pm.N)) for _ in range(cnt))      # noqa: E731
    ins = [gpu.to_device(x) for x in (rb(32 * nb), wit(pv.a_L), wit(pv.a_R), wit(pv.a_O), rb(32 * nb), scal(nb * NVALS), scal(nb * 8))]
    outs = [gpu.malloc(s) for s in (64 * nb * (11 + 2 * k), 160 * nb)]
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    st = C.c_void_p(gpu.stream())
    ts = []
    for step in range(WARM + STEPS):
        assert hip.hipEventRecord(ev[0], st) == 0
        gpu.r1cs_prove_fs_dev(gens, circ, nb, ins[0], ins[1], ins[2], ins[3], ins[6], outs[0], outs[1], d_v_blinding=ins[5],
                              d_vector_keys=ins[4])
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


def child(what, nb):
    if what == "dev":
        print("RESULT", fmt(device(nb)))
    else:
        ts, proofs = mirror(nb, what == "fused")
        import hashlib
        print("RESULT", fmt(ts), hashlib.sha256(proofs).hexdigest(), statistics.median(ts))


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]))
    lines = [f"# tools/bench_prove_fs.py   {NVALS} x {NBITS}-bit range provers (n = {N_MUL}, m = {NVALS}); per shape and route a fresh process, "
             f"{WARM} warm-up + {STEPS} timed steps: median (min..max) ms",
             "# nb     dev: prove_fs_dev, HIP events        fused: prove_batch, wall clock       staged: prove_batch, wall clock      staged/fused"]
    for nb in (256, 1, 16):
        res = {}
        for what in ("dev", "fused", "staged"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(nb)], capture_output=True, text=True, timeout=900)
            got = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
            assert out.returncode == 0 and got, (what, nb, out.stdout[-2000:], out.stderr[-2000:])
            res[what] = got[0][len("RESULT "):]
        f, s = res["fused"].rsplit(" ", 2), res["staged"].rsplit(" ", 2)
        assert f[1] == s[1], "the fused and the staged route disagree on the proof bytes"
        lines.append(f"{nb:<6d} {res['dev']}   {f[0]}   {s[0]}   {float(s[2]) / float(f[2]):8.2f}")
        print(lines[-1])
        sys.stdout.flush()
    path = os.path.join(ROOT, "profiles", "prove_fs.log")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
