#!/usr/bin/env python3
"""bpgpu_r1cs_prove_values (one call: commitments, verdicts and proofs from the provers' committed values) against the chain of
host-form calls it replaces, wall clock from the first call to the drained stream.  Writes profiles/prove_values.log, the source of
every figure that include/bpgpu.h, README.md, DESIGN.md and INTEGRATION.md quote on this call.

  one     the one call in host form, operands and results in pageable memory or in bpgpu_host_alloc memory (pinned); the witness
          planes are not asked for
  chain   one-phase: r1cs_commit_values -> r1cs_witness_synthesize -> r1cs_constraints_satisfied -> r1cs_prove_fs
          two-phase: r1cs_commit_values -> r1cs_prove_fs2 (with the witness outputs) -> r1cs_constraints_satisfied
          on the same kind of memory.  Both legs call the C entry points themselves on buffers made once, outside the timed steps.
          The chain is the baseline, so it does not come from the tree under test: --baseline ROOT names a built checkout of the
          parent commit, whose package and test helpers the chain's process imports.  Without --baseline the chain lines are UNMEASURED.
  pool    the range shape on a {0, 0} pool: bpgpu_pool_r1cs_prove_values against r1cs_witness_synthesize (host call, slot 0's context)
          followed by bpgpu_pool_r1cs_prove_fs on the planes it returned, both timed (that baseline commits nothing and checks nothing)
  clear   the clearing launch alone, from the library's own events (kind 22: the last interval of that kind of a call)

Shapes: 256 provers x 16 x 64-bit range values (n = 1024, m = 16); 256 x shuffle 64; 1 x shuffle 2^10.  Blinding vectors from keys.
A fresh process per line, WARM untimed steps, then STEPS timed ones: median (min..max) ms.  The rule of profiles/witness_synth.log: the
one call is faster where its MAXIMUM lies below the chain's MINIMUM; overlapping spans are reported as such."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, STEPS = 3, 20
SHAPES = {"range": (256, "range", 64, 16), "shuffle64": (256, "shuffle", 64, 0), "shuffle1024": (1, "shuffle", 1 << 10, 0)}


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):8.3f}..{max(ts):9.3f})"


def setup(root, shape):
    """the case, its operands for nb provers (every prover the case's prover 0 under its own blindings) and the CSR of its circuit"""
    sys.path[:0] = [root, os.path.join(root, "tests"), os.path.join(root, "oracle")]
    import random
    import witness_cases as wc
    nb, kind, a, b = SHAPES[shape]
    case = wc.range_case(a, b) if kind == "range" else wc.shuffle_case(a)
    prog = case.prog
    two = prog.nchi == 1
    rnd = random.Random(len(shape))
    rb = lambda cnt: bytes(rnd.getrandbits(8) for _ in range(cnt))      # noqa: E731
    scal = lambda cnt: b"".join(wc.mont(rnd.randrange(wc.N)) for _ in range(cnt))      # noqa: E731
    v, inputs, _ = case.prover(0)
    ops = dict(init_states=rb(32 * nb), v=b"".join(wc.mont(x % wc.N) for x in v) * nb, v_blinding=scal(nb * prog.m), inputs=None,
               blindings=scal(nb * (11 if two else 8)), vector_keys=rb(nb * (64 if two else 32)),
               gadget_label=wc.SHUFFLE_LABEL if two else None)
    return wc, case, nb, ops, wc.circuit_csr(case)


def make(maker, case, csr):
    q, nchi, rp, kd, ix, cf = csr
    prog = case.prog
    circ = maker.circuit_create_param(q, 1, rp, kd, ix, cf, prog.n, prog.m) if nchi else maker.circuit_create(rp, kd, ix, cf, prog.n, prog.m)
    return circ, maker.witness_create(*prog.create_args())


def timed(step, check=None):
    """the wall clock of step() alone; check() looks at its results outside the timing"""
    ts = []
    for i in range(WARM + STEPS):
        t0 = time.perf_counter()
        step()
        t1 = time.perf_counter()
        if check:
            check()
        if i >= WARM:
            ts.append((t1 - t0) * 1e3)
    return ts


def child(leg, shape, root):
    """one leg in this process.  Every call is the C entry point itself on buffers made once, outside the timed steps -- what a C or
    Rust host pays -- not the Python binding's methods, which copy every result into a bytes object"""
    import ctypes as C
    wc, case, nb, ops, csr = setup(root, shape)
    import oracle_lib as o
    import mpc_bulletproof_amd as m
    lib = m.lib._lib
    leg, pinned = (leg[:-len("-pinned")], True) if leg.endswith("-pinned") else (leg, False)
    prog = case.prog
    n, mm, q, two = prog.n, prog.m, csr[0], prog.nchi == 1
    k = max(n - 1, 0).bit_length()
    cap = 1 << k
    G, H = o.gens("G", cap), o.gens("H", cap)

    def mem(size, data=None):
        """an operand or a result in page-locked or in pageable memory"""
        if pinned:
            return m.lib.host_alloc(max(size, 1), data)
        return (C.c_uint8 * max(size, 1)).from_buffer_copy(data) if data is not None else (C.c_uint8 * max(size, 1))()
    i = {key: mem(len(ops[key]), ops[key]) for key in ("init_states", "v", "v_blinding", "blindings", "vector_keys")}
    label = C.c_char_p((ops["gadget_label"] + bytes(32))[:32]) if two else None
    sizes = dict(V=64 * nb * mm, Vc=32 * nb * mm, st=32 * nb, pts=64 * nb * (11 + 2 * k), sc=160 * nb,
                 wire=nb * (1 + (14 if two else 11) * 32 + (2 * k + 2) * 32), ch=32 * nb * (5 + k), so=32 * nb, chi=32 * nb,
                 aL=32 * nb * n, aR=32 * nb * n, aO=32 * nb * n)
    r = {key: mem(size) for key, size in sizes.items()}
    ok, row, gate = (C.c_int32 * nb)(), (C.c_int64 * nb)(), (C.c_int64 * nb)()
    chi = r["chi"] if two else None

    def ck(rc):
        assert rc == 0, rc

    def accepted():
        assert list(ok) == [1] * nb
        ok[0] = 0
    out = {}
    if leg in ("one", "chain", "clear"):
        gpu = m.BpGpu(0)
        ctx = gpu.ctx
        gens = gpu.gens_create(G, H, o.generator(), o.generator(), 8)
        circ, w = make(gpu, case, csr)
        if leg == "chain":
            def step():
                ck(lib.bpgpu_r1cs_commit_values(ctx, gens, nb, mm, i["v"], i["v_blinding"], i["init_states"], r["V"], r["Vc"], r["st"]))
                if two:
                    ck(lib.bpgpu_r1cs_prove_fs2(ctx, gens, circ, w, nb, r["st"], label, i["v"], None, None, None, i["vector_keys"], i["v_blinding"],
                                                i["blindings"], r["pts"], r["sc"], r["wire"], r["ch"], r["so"], chi, r["aL"], r["aR"], r["aO"]))
                    ck(lib.bpgpu_r1cs_constraints_satisfied(ctx, circ, nb, r["aL"], r["aR"], r["aO"], i["v"], chi, ok, row, gate, None))
                else:
                    ck(lib.bpgpu_r1cs_witness_synthesize(ctx, w, nb, 0, i["v"], None, None, r["aL"], r["aR"], r["aO"]))
                    ck(lib.bpgpu_r1cs_constraints_satisfied(ctx, circ, nb, r["aL"], r["aR"], r["aO"], i["v"], None, ok, row, gate, None))
                    ck(lib.bpgpu_r1cs_prove_fs(ctx, gens, circ, nb, r["st"], r["aL"], r["aR"], r["aO"], None, None, i["vector_keys"],
                                               i["v_blinding"], i["blindings"], r["pts"], r["sc"], r["wire"], r["ch"], r["so"]))
        else:
            def step():
                ck(lib.bpgpu_r1cs_prove_values(ctx, gens, circ, w, nb, i["init_states"], label, i["v"], i["v_blinding"], None, None, None,
                                               i["vector_keys"], i["blindings"], r["V"], r["Vc"], ok, row, gate, r["pts"], r["sc"], r["wire"],
                                               r["ch"], r["so"], chi, None, None, None))
        if leg == "clear":
            # (profiling adds its own events: this leg times nothing but the launch it asks about)
            gpu.profile_enable(True)
            epoch = gpu.profile_epoch()
            ts = []
            for j in range(WARM + STEPS):
                step()
                accepted()
                last = [b - a for kind, a, b in gpu.profile_intervals(epoch) if kind == m.lib.PROF_NAMES[22]][-1]
                if j >= WARM:
                    ts.append(last)
            out["ms"] = ts
        else:
            out["ms"] = timed(step, accepted)
    else:
        pool = m.BpPool([0, 0])
        gens = pool.gens_create(G, H, o.generator(), o.generator(), 8)
        if leg == "pool-one":
            circ, w = make(pool, case, csr)

            def step():
                ck(lib.bpgpu_pool_r1cs_prove_values(pool.pool, gens, circ, w, nb, i["init_states"], label, i["v"], i["v_blinding"], None, None,
                                                    None, i["vector_keys"], i["blindings"], r["V"], r["Vc"], ok, row, gate, r["pts"], r["sc"],
                                                    r["wire"], r["ch"], r["so"], chi, None, None, None))
        else:               # pool-chain: on any tree that has the pool
            _, _, rp, kd, ix, cf = csr
            circ = pool.circuit_create(rp, kd, ix, cf, n, mm)
            g0 = pool.ctx(0)
            w = g0.witness_create(*prog.create_args())
            ck(lib.bpgpu_r1cs_commit_values(g0.ctx, pool.gens_get(gens, 0), nb, mm, i["v"], i["v_blinding"], i["init_states"], r["V"], r["Vc"],
                                            r["st"]))

            def step():
                ck(lib.bpgpu_r1cs_witness_synthesize(g0.ctx, w, nb, 0, i["v"], None, None, r["aL"], r["aR"], r["aO"]))
                ck(lib.bpgpu_pool_r1cs_prove_fs(pool.pool, gens, circ, nb, r["st"], r["aL"], r["aR"], r["aO"], None, None, i["vector_keys"],
                                                i["v_blinding"], i["blindings"], r["pts"], r["sc"], r["wire"], r["ch"], r["so"]))
        out["ms"] = timed(step, accepted if leg == "pool-one" else None)      # (the pool's baseline checks nothing: no verdicts)
    print("RESULT", json.dumps(out))
    sys.stdout.flush()
    os._exit(0)          # (the handles die with the process)


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3], sys.argv[4])
    baseline = None
    if "--baseline" in sys.argv:
        baseline = os.path.abspath(sys.argv[sys.argv.index("--baseline") + 1])

    def run(leg, shape, root):
        if root is None:
            return None
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, shape, root], capture_output=True, text=True, timeout=900)
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
        assert out.returncode == 0 and got, (leg, shape, out.stdout[-2000:], out.stderr[-2000:])
        return json.loads(got[0][len("RESULT "):])["ms"]
    lines = [f"# tools/bench_prove_values.py   wall clock of one batch, host form, first call to drained stream; a fresh process per line, {WARM} "
             f"warm-up + {STEPS} timed steps: median (min..max) ms",
             "# chain = the host-form calls the one call replaces, timed on a build of the PARENT commit"
             + ("" if baseline else " -- no --baseline given: UNMEASURED"),
             "# verdict: the one call is faster where its max lies below the chain's min; else the spans overlap (or the chain is faster)"]

    def emit(text):
        lines.append(text)
        print(text)
        sys.stdout.flush()

    def verdict(one, chain):
        if chain is None:
            return "chain UNMEASURED"
        if max(one) < min(chain):
            return f"one call faster: max {max(one):.3f} < chain min {min(chain):.3f}; medians differ by {statistics.median(chain) - statistics.median(one):.3f} ms"
        if max(chain) < min(one):
            return f"CHAIN faster: max {max(chain):.3f} < one call's min {min(one):.3f}"
        return "spans OVERLAP: no difference claimed"
    for shape, (nb, kind, a, b) in SHAPES.items():
        what = f"{nb} x {b} x {a}-bit range (n = {64 * 16}, m = 16)" if kind == "range" else f"{nb} x shuffle {a} (n = {2 * a - 2}, m = {2 * a})"
        one, chain = run("one", shape, HERE), run("chain", shape, baseline)
        emit(f"{shape:12s} {what}")
        emit(f"  one   pageable   {fmt(one)}")
        emit(f"  chain pageable   {fmt(chain) if chain else 'UNMEASURED'}")
        emit(f"  -> {verdict(one, chain)}")
        pin, cpin = run("one-pinned", shape, HERE), run("chain-pinned", shape, baseline)
        emit(f"  one   pinned     {fmt(pin)}")
        emit(f"  chain pinned     {fmt(cpin) if cpin else 'UNMEASURED'}")
        emit(f"  -> {verdict(pin, cpin)}")
    pone, pchain = run("pool-one", "range", HERE), run("pool-chain", "range", baseline)
    emit("pool {0, 0}   the range shape; baseline: r1cs_witness_synthesize (host) + bpgpu_pool_r1cs_prove_fs, no commitments, no check")
    emit(f"  one   pageable   {fmt(pone)}")
    emit(f"  chain pageable   {fmt(pchain) if pchain else 'UNMEASURED'}")
    emit(f"  -> {verdict(pone, pchain)}")
    clear = run("clear", "range", HERE)
    emit(f"clear        the clearing launch at 256 provers (range shape, nobody rejected), kind 22 events: {fmt(clear)}")
    path = os.path.join(HERE, "profiles", "prove_values.log")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
