#!/usr/bin/env python3
"""bpgpu_r1cs_constraints_satisfied_dev beside the proof it guards and the host loop it replaces.  Writes
profiles/constraints_satisfied.log (the source of the figures in DESIGN.md), one block per shape:

  range    256 provers, each range-proving 16 values of 64 bits in one constraint system (n = 1024, q = 2064, m = 16: the r1cs_prove
           shape of BASELINE.json);
  shuffle  one prover of the 2^14-shuffle as a parametric circuit (n = 32766, m = 32768, one gadget challenge).

Per shape, in one process: `check` = the _dev call on resident operands (all four results asked for; `check-ok` = ok alone), `prove`
= bpgpu_r1cs_prove_fs_dev (range) or _fs2_begin_dev + _finish_dev (shuffle) on the same buffers, HIP events on the context's stream
around each call; `host` = the host mirror's Prover::constraints_satisfied() loop over the same provers, wall clock
(tools/bench_satisfied_host.cpp; a shuffle prover holds no rows before Prover::prove runs its deferred phase, so that loop has nothing
to walk there).  WARM untimed steps, then STEPS timed ones: median (min..max) ms.  --shuffle-k K runs a smaller shuffle."""
import ctypes as C
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

WARM, STEPS = 3, 20
NVALS, NBITS, NB = 16, 64, 256


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):8.3f}..{max(ts):9.3f})"


class Timer:
    def __init__(self, gpu):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0
        self.st = C.c_void_p(gpu.stream())

    def run(self, call):
        ts = []
        for step in range(WARM + STEPS):
            assert self.hip.hipEventRecord(self.ev[0], self.st) == 0
            call()
            assert self.hip.hipEventRecord(self.ev[1], self.st) == 0 and self.hip.hipEventSynchronize(self.ev[1]) == 0
            ms = C.c_float()
            assert self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
            if step >= WARM:
                ts.append(ms.value)
        return ts


def report(lines, name, check, check_ok, prove):
    c, p = statistics.median(check), statistics.median(prove)
    lines.append(f"{name:8s} check     {fmt(check)}")
    lines.append(f"{name:8s} check-ok  {fmt(check_ok)}")
    lines.append(f"{name:8s} prove     {fmt(prove)}")
    verdict = "MORE than a tenth of the proof it guards" if c > p / 10 else "less than a tenth of the proof it guards"
    lines.append(f"{name:8s} check / prove = {c / p:.4f}: {verdict}")


def device_range(lines):
    import mpc_dealer as md
    import oracle_lib as o
    import pymodel as pm
    import mpc_bulletproof_amd as m
    n, nb = NVALS * NBITS, NB
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"RangeProofTest"))
    pv.pc_gens.commit = lambda v, b: pm.G           # the commitments play no part here: skip the model's scalar multiplications
    for i in range(NVALS):
        v = (0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1)
        _, var = pv.commit(v, 1)
        pm.range_proof_gadget(pv, pm.lc_var(var), v, NBITS)
    rp, kd, ix, cf, _ = md.circuit_rows(pv.constraints)
    q = len(pv.constraints)
    lens = [rp[r + 1] - rp[r] for r in range(q)]
    rnd = random.Random(nb)
    rb = lambda cnt: bytes(rnd.getrandbits(8) for _ in range(cnt))      # noqa: E731
    wit = lambda v: b"".join(md.mont(x) for x in v) * nb               # noqa: E731
    scal = lambda cnt: b"".join(md.mont(rnd.randrange(pm.N)) for _ in range(cnt))      # noqa: E731
    k = (n - 1).bit_length()
    gpu = m.BpGpu(0)
    gens = gpu.gens_create(o.gens("G", n), o.gens("H", n), o.generator(), o.generator(), 8)
    circ = gpu.circuit_create(rp, kd, ix, cf, n, NVALS)
    ins = [gpu.to_device(x) for x in (rb(32 * nb), wit(pv.a_L), wit(pv.a_R), wit(pv.a_O), rb(32 * nb), scal(nb * NVALS), scal(nb * 8), wit(pv.v))]
    outs = [gpu.malloc(s) for s in (64 * nb * (11 + 2 * k), 160 * nb, 4 * nb, 8 * nb, 8 * nb, 32 * nb * q)]
    t = Timer(gpu)
    check = t.run(lambda: gpu.r1cs_constraints_satisfied_dev(circ, nb, ins[1], ins[2], ins[3], outs[2], d_v=ins[7], d_first_bad_row=outs[3],
                                                             d_first_bad_gate=outs[4], d_residuals=outs[5]))
    check_ok = t.run(lambda: gpu.r1cs_constraints_satisfied_dev(circ, nb, ins[1], ins[2], ins[3], outs[2], d_v=ins[7]))
    assert gpu.input_flag() == 0 and gpu.download(outs[2], 4 * nb) == (1).to_bytes(4, "little") * nb
    prove = t.run(lambda: gpu.r1cs_prove_fs_dev(gens, circ, nb, ins[0], ins[1], ins[2], ins[3], ins[6], outs[0], outs[1], d_v_blinding=ins[5],
                                                d_vector_keys=ins[4]))
    assert gpu.input_flag() == 0
    lines.append(f"# range: nb = {nb}, n = {n}, m = {NVALS}, q = {q}, {rp[-1]} terms, rows of {min(lens)}..{max(lens)} terms")
    report(lines, "range", check, check_ok, prove)
    for p in ins + outs:
        gpu.free(p)
    gpu.circuit_destroy(circ)
    gpu.gens_destroy(gens)
    gpu.close()


def shuffle_model(ks):
    """the k-shuffle as a parametric circuit and one prover's witness from the model's gadget (minutes of Python at k = 2^14: kept in
    tools/_wl/ between runs)"""
    import pickle
    import mpc_dealer as md
    import pymodel as pm
    path = os.path.join(ROOT, "tools", "_wl", "satisfied_shuffle_%d.pkl" % ks)
    if os.path.exists(path):
        with open(path, "rb") as fh:
            return pickle.load(fh)
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"ShuffleProofTest"))
    pv.pc_gens.commit = lambda v, b: pm.G
    xs = [((0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1)) for i in range(ks)]
    vars_ = [pv.commit(v, 1)[1] for v in xs + xs[1:] + xs[:1]]
    pm.shuffle_gadget(pv, vars_[:ks], vars_[ks:])
    pv._create_randomized_constraints()
    assert len(pv.a_L) == 2 * (ks - 1)
    out = md.circuit_rows(pv.constraints, param=True) + (list(pv.a_L), list(pv.a_R), list(pv.a_O), list(pv.v), len(pv.constraints))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as fh:
        pickle.dump(out, fh)
    return out


def device_shuffle(lines, ks):
    import mpc_dealer as md
    import oracle_lib as o
    import pymodel as pm
    import mpc_bulletproof_amd as m
    nb, n, mm = 1, 2 * (ks - 1), 2 * ks
    rp, kd, ix, cf, chi, a_L, a_R, a_O, vals, q = shuffle_model(ks)
    rnd = random.Random(ks)
    rb = lambda cnt: bytes(rnd.getrandbits(8) for _ in range(cnt))      # noqa: E731
    wit = lambda v: b"".join(md.mont(x) for x in v)                    # noqa: E731
    scal = lambda cnt: b"".join(md.mont(rnd.randrange(pm.N)) for _ in range(cnt))      # noqa: E731
    k = (n - 1).bit_length()
    gpu = m.BpGpu(0)
    gens = gpu.gens_create(o.gens("G", 1 << k), o.gens("H", 1 << k), o.generator(), o.generator(), 8)
    circ = gpu.circuit_create_param(q, 1, rp, kd, ix, cf, n, mm)
    ins = [gpu.to_device(x) for x in (rb(32), scal(3), wit(a_L), wit(a_R), wit(a_O), rb(32), scal(mm), scal(8), wit(vals), md.le(chi))]
    outs = [gpu.malloc(s) for s in (64 * (11 + 2 * k), 160, 4, 8, 8, 32 * q)]
    t = Timer(gpu)
    check = t.run(lambda: gpu.r1cs_constraints_satisfied_dev(circ, nb, ins[2], ins[3], ins[4], outs[2], d_v=ins[8], d_gadget_challenges=ins[9],
                                                             d_first_bad_row=outs[3], d_first_bad_gate=outs[4], d_residuals=outs[5]))
    check_ok = t.run(lambda: gpu.r1cs_constraints_satisfied_dev(circ, nb, ins[2], ins[3], ins[4], outs[2], d_v=ins[8], d_gadget_challenges=ins[9]))
    assert gpu.input_flag() == 0 and gpu.download(outs[2], 4) == (1).to_bytes(4, "little")

    def prove():
        sess = gpu.r1cs_prove_fs2_begin_dev(gens, circ, nb, 0, ins[0], b"shuffle challenge", ins[1])
        gpu.r1cs_prove_fs2_finish_dev(gens, circ, sess, ins[2], ins[3], ins[4], ins[7], outs[0], outs[1], d_v_blinding=ins[6], d_vector_keys=ins[5])
    pr = t.run(prove)
    assert gpu.input_flag() == 0
    lens = [sum(rp[j * q + r + 1] - rp[j * q + r] for j in range(2)) for r in range(q)]
    lines.append(f"# shuffle: nb = 1, k = {ks}, n = {n}, m = {mm}, q = {q}, {rp[-1]} terms, rows of {min(lens)}..{max(lens)} terms")
    report(lines, "shuffle", check, check_ok, pr)
    for p in ins + outs:
        gpu.free(p)
    gpu.circuit_destroy(circ)
    gpu.gens_destroy(gens)
    gpu.close()


def host_loop(lines):
    exe = os.path.join(ROOT, "tools", "_wl", "bench_satisfied_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    pkg = os.path.join(ROOT, "mpc_bulletproof_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(pkg, "host"), "-I" + os.path.join(ROOT, "tests", "host"),
                           "-o", exe, os.path.join(ROOT, "tools", "bench_satisfied_host.cpp"), "-L" + pkg, "-lbphost", "-lbpgpu",
                           "-Wl,-rpath," + pkg])
    out = subprocess.run([exe, str(NB), str(NVALS), str(NBITS), str(WARM + STEPS)], capture_output=True, text=True, timeout=900)
    ts = [float(ln.split()[1]) for ln in out.stdout.splitlines() if ln.startswith("MS")]
    assert out.returncode == 0 and len(ts) == WARM + STEPS, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    lines.append(f"range    host      {fmt(ts[WARM:])}   Prover::constraints_satisfied() over the {NB} provers, one thread, wall clock")


def child(what, arg):
    lines = []
    {"range": lambda: device_range(lines), "shuffle": lambda: device_shuffle(lines, arg), "host": lambda: host_loop(lines)}[what]()
    for ln in lines:
        print("RESULT " + ln)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]))
    ks = int(sys.argv[sys.argv.index("--shuffle-k") + 1]) if "--shuffle-k" in sys.argv else 1 << 14
    lines = [f"# tools/bench_satisfied.py   a fresh process per shape, {WARM} warm-up + {STEPS} timed steps per call: median (min..max) ms; "
             "check, prove: HIP events around the _dev calls on resident operands"]
    for what, arg in (("range", 0), ("host", 0), ("shuffle", ks)):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, str(arg)], capture_output=True, text=True, timeout=1100)
        got = [ln[len("RESULT "):] for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        assert out.returncode == 0 and got, (what, out.stdout[-2000:], out.stderr[-2000:])
        lines += got
        print("\n".join(got))
        sys.stdout.flush()
    path = os.path.join(ROOT, "profiles", "constraints_satisfied.log")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
