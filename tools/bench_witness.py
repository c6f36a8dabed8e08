#!/usr/bin/env python3
"""Witness synthesis on the device (bpgpu_r1cs_witness_synthesize_dev) and the one-call two-phase prover (bpgpu_r1cs_prove_fs2_dev)
against the two calls around a host that evaluates the gadget.  Appends a run to profiles/witness_synth.log (the source of the figures in
DESIGN.md "Witness synthesis"; the earlier runs stay).  Shapes: 256 provers x 16 x 64-bit range (one level of 1024 BIT gates), 256
provers x shuffle k = 64 (two chains of 63 dependent gates: a head and 62 members), 1 prover x shuffle k = 2^14 (two chains of 16 383).

  synth   the synthesis alone on resident operands, HIP events around the call, on the launch forms (BPGPU_OPT_WITNESS_ROUTE 1 = a
          lane per prover, 2 = a block per prover; route 0 with BPGPU_OPT_WITNESS_SCAN_MIN 1 = a block per prover with the product
          chains scanned, for the shapes that have a chain) and what bpgpu_witness_plan picks; next to it the HOST's evaluation of the
          same gates: this tool's Python integers (a Rust host is faster: the figure bounds the host from above);
  sweep   the same for ONE shuffle whose two chains have 8 .. 16 382 members, for 1 and 256 provers, block form against scan form:
          where BPGPU_OPT_WITNESS_SCAN_MIN's default is read from -- the smallest power of two >= 16 from which on the scan's
          MAXIMUM lies below the block form's MINIMUM for both batch sizes -- and one line of 4096 x shuffle k = 64 on all three
          forms, beyond the 1024 blocks that are resident at once;
  prove   bpgpu_r1cs_prove_fs2_dev (one call) against bpgpu_r1cs_prove_fs2_begin_dev + the host's gadget (download of the challenge,
          evaluation, Montgomery encoding, upload) + _finish_dev on the same inputs, wall clock from the first call to the drained
          stream; `chains` is the pair of _dev calls alone on a resident phase-2 witness, the figure tools/bench_prove_fs2.py
          reports (profiles/prove_fs2.log holds it for the parent commit).  Shapes: 256 x shuffle k = 64 and 1 x shuffle k = 2^10 -- the
          largest single prover that tool proves through this binding; the k = 2^14 prover (generator tables for 2^15) goes through
          the host mirror (tools/bench_shuffle.py), which is out of scope here, so that shape has the synthesis line alone.  The
          range shape is a one-phase prover: bpgpu_r1cs_prove_fs_dev after the synthesis, no second call to save.


`bench_witness.py affine` measures the affine chains instead and appends to profiles/witness_affine.log: the two shuffle lines again
(the product kernel is meant to be unchanged: each span is compared with the last run of profiles/witness_synth.log, widened by the
8 % box spread DESIGN.md gives for that log), then ONE Horner pair per prover (tests/witness_affine_cases.py: two affine chains of
8 .. 16 382 members) for 1 and 256 provers, block form against scan form.  The block form is the path these programs took before
there was an affine scan.  WIT_AFFINE_MIN (csrc/bpgpu_internal.h) is read from that sweep by the rule of the shuffle sweep.

`bench_witness.py inv` measures the INV gates (BPGPU_GATE_INV) and appends to profiles/witness_inv.log.  Shapes: 256 provers x one
level of 1024 INV gates, 1 x 1024, 4096 x 16, and 256 x a chain of 64 INV gates each reading the previous a_O (one gate a level:
nothing to batch).  Per shape three columns: (a) the block form (BPGPU_OPT_WITNESS_ROUTE 2: one inversion per thread and level),
(b) the lane form (route 1: one inversion per gate) -- the A/B of the batching on one commit --, and (c) the same program with every
INV gate replaced by an INPUT gate fed the precomputed pairs, on route 2: the only way a library without the op runs it, the host's
own inversions and the upload of the pairs left out; what the device inversion costs over having been handed the answer is (a) / (c).

`bench_witness.py divrem` measures the DIVREM gates (BPGPU_GATE_DIVREM) and appends to profiles/witness_divrem.log.  The shapes of
`inv`, each on two kinds of operands: `u64` = x of 64 bits over y of 33 bits, both below 2^64 (a 32.32 fixed-point quotient: 32 steps
of the division), and `wide` = x of 252 bits over y of 128 bits (125 steps, the long loop).  Per line four columns: (a) the block
form and (b) the lane form of the program with DIVREM gates, and (c), (d) the same two forms of the same program with every DIVREM
gate replaced by an INPUT gate handed the (q, r) pairs, the host's divisions and the upload left out: the floor.

A fresh process per line under its own time limit; WARM untimed steps, then STEPS timed ones, medians (min..max) in ms."""
import ctypes as C
import json
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
STEP_LIMIT = 420          # seconds per child process


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):8.3f}..{max(ts):9.3f})"


def shuffle_program(k):
    """the shuffle's gates (tests/witness_cases.py) and one prover's values"""
    import witness_cases as wc
    prog = wc.Program(2 * k, nchi=1)
    prog.end_phase1()
    wc._shuffle_gates(prog, k, 0)
    xs = [((0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1)) for i in range(k)]
    return prog, xs + xs[1:] + xs[:1]


def horner_program(k):
    """the Horner gadget's gates (tests/witness_affine_cases.py: two affine chains of k - 2 members) and one prover's values"""
    import witness_cases as wc
    import witness_affine_cases as ac
    prog = wc.Program(2 * k, nchi=1)
    prog.end_phase1()
    ac._horner_gates(prog, k, 0)
    xs = [((0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1)) for i in range(k)]
    return prog, xs + xs


def range_program(bits, m):
    import witness_cases as wc
    case = wc.range_case(bits, m)
    return case.prog, [((0x9E3779B97F4A7C15 * (i + 1)) & ((1 << bits) - 1)) for i in range(m)]


INV_SHAPES = (("level", 256, 1024), ("level", 1, 1024), ("level", 4096, 16), ("chain", 256, 64))


def inv_programs(shape, size):
    """(the program with INV gates, its twin with INPUT gates, one prover's values): `level` = size independent gates inv(v_j + i + 1),
    `chain` = size gates inv(a_O[i - 1] + v_j)"""
    import witness_cases as wc
    import witness_inv_cases as ic
    m = 4
    prog, twin = ic.Program(m), ic.Program(m)
    last = None
    for i in range(size):
        if shape == "chain" and last is not None:
            last = prog.inv([(wc.O, last, 1), (wc.V, i % m, 1)])
        else:
            last = prog.inv([(wc.V, i % m, 1), (wc.ONE, 0, i + 1)])
        twin.input()
    prog.end_phase1()
    twin.end_phase1()
    return prog, twin, [((0x9E3779B97F4A7C15 * (i + 1)) & ((1 << 64) - 1)) for i in range(m)]


def inv_synth(shape, nb, size):
    import mpc_dealer as md
    import mpc_bulletproof_amd as m
    prog, twin, v = inv_programs(shape, size)
    want = prog.evaluate(v)
    assert all(x for x in want[0]) and want[2] == [1] * size
    gpu = m.BpGpu(0)
    d_v = gpu.to_device(b"".join(md.mont(x) for x in v) * nb)
    d_in = gpu.to_device(b"".join(md.mont(x) for pair in zip(want[0], want[1]) for x in pair) * nb)
    planes = [gpu.malloc(32 * nb * size) for _ in range(3)]
    timer = Timer(gpu)
    out = {}
    for col, which, route in (("block", prog, 2), ("lane", prog, 1), ("input", twin, 2)):
        w = gpu.witness_create(*which.create_args())
        gpu.set_option("witness_route", route)
        ts = []
        for step in range(WARM + STEPS):
            ms = timer.events(lambda: gpu.r1cs_witness_synthesize_dev(w, nb, 0, *planes, d_v=d_v, d_inputs=d_in if which is twin else None))
            if step >= WARM:
                ts.append(ms)
        assert gpu.input_flag() == 0
        for k in range(3):
            got = gpu.download(planes[k], 32 * nb * size)
            assert got[-32 * size:] == b"".join(md.mont(x) for x in want[k]), "the device's witness differs from the host's"
        gpu.witness_destroy(w)
        out[col] = ts
    a, b, c = (statistics.median(out[col]) for col in ("block", "lane", "input"))
    plan = m.lib.witness_plan(*prog.plan_args(), nb)
    return (f"(a) block {fmt(out['block'])}   (b) lane {fmt(out['lane'])}   (c) INPUT {fmt(out['input'])}   (b)/(a) {b / a:8.2f}   (a)/(c) {a / c:8.2f}   "
            f"(b)/(c) {b / c:8.2f}   plan: {('lane', 'block', 'scan')[plan['route1'] - 1]:5s}   levels {plan['levels1']:3d}")


DIVREM_OPERANDS = {"u64": (64, 33), "wide": (252, 128)}      # bit lengths of x and y


def divrem_programs(shape, size, kind):
    """(the program with DIVREM gates, its twin with INPUT gates, one prover's values): `level` = size independent gates
    divrem(v_x + i + 1, v_y), `chain` = size gates divrem(v_x + a_R[i - 1], v_y), each reading the remainder below it"""
    import witness_cases as wc
    import witness_divrem_cases as dc
    bx, by = DIVREM_OPERANDS[kind]
    v = [(1 << (bx - 1)) | ((0x9E3779B97F4A7C15 * (j + 1)) & ((1 << (bx - 2)) - 1)) for j in range(2)]
    v += [(1 << (by - 1)) | ((0xC2B2AE3D27D4EB4F * (j + 1)) & ((1 << (by - 2)) - 1)) for j in range(2)]
    prog, twin = dc.Program(4), dc.Program(4)
    last = None
    for i in range(size):
        if shape == "chain" and last is not None:
            last = prog.divrem([(wc.V, i % 2, 1), (wc.R, last, 1)], [(wc.V, 2 + i % 2, 1)])
        else:
            last = prog.divrem([(wc.V, i % 2, 1), (wc.ONE, 0, i + 1)], [(wc.V, 2 + i % 2, 1)])
        twin.input()
    prog.end_phase1()
    twin.end_phase1()
    return prog, twin, v


def divrem_synth(shape, nb, size, kind):
    import mpc_dealer as md
    import mpc_bulletproof_amd as m
    prog, twin, v = divrem_programs(shape, size, kind)
    want = prog.evaluate(v)
    bx, by = DIVREM_OPERANDS[kind]
    assert all(q.bit_length() in (bx - by, bx - by + 1) for q in want[0])
    gpu = m.BpGpu(0)
    d_v = gpu.to_device(b"".join(md.mont(x) for x in v) * nb)
    d_in = gpu.to_device(b"".join(md.mont(x) for pair in zip(want[0], want[1]) for x in pair) * nb)
    planes = [gpu.malloc(32 * nb * size) for _ in range(3)]
    timer = Timer(gpu)
    out = {}
    for col, which, route in (("block", prog, 2), ("lane", prog, 1), ("input block", twin, 2), ("input lane", twin, 1)):
        w = gpu.witness_create(*which.create_args())
        gpu.set_option("witness_route", route)
        ts = []
        for step in range(WARM + STEPS):
            ms = timer.events(lambda: gpu.r1cs_witness_synthesize_dev(w, nb, 0, *planes, d_v=d_v, d_inputs=d_in if which is twin else None))
            if step >= WARM:
                ts.append(ms)
        assert gpu.input_flag() == 0
        for k in range(3):
            got = gpu.download(planes[k], 32 * nb * size)
            assert got[-32 * size:] == b"".join(md.mont(x) for x in want[k]), "the device's witness differs from divmod's"
        gpu.witness_destroy(w)
        out[col] = ts
    a, b, c, d = (statistics.median(out[col]) for col in ("block", "lane", "input block", "input lane"))
    plan = m.lib.witness_plan(*prog.plan_args(), nb)
    return (f"(a) block {fmt(out['block'])}   (b) lane {fmt(out['lane'])}   (c) INPUT block {fmt(out['input block'])}   "
            f"(d) INPUT lane {fmt(out['input lane'])}   (a)/(c) {a / c:8.2f}   (b)/(d) {b / d:8.2f}   "
            f"plan: {('lane', 'block', 'scan')[plan['route1'] - 1]:5s}   levels {plan['levels1']:3d}")


class Timer:
    def __init__(self, gpu):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            assert self.hip.hipEventCreate(C.byref(e)) == 0
        self.st = C.c_void_p(gpu.stream())

    def events(self, body):
        assert self.hip.hipEventRecord(self.ev[0], self.st) == 0
        body()
        assert self.hip.hipEventRecord(self.ev[1], self.st) == 0 and self.hip.hipEventSynchronize(self.ev[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return ms.value


FORMS = {"lane": (1, 0), "block": (2, 0), "scan": (0, 1)}      # form -> (BPGPU_OPT_WITNESS_ROUTE, BPGPU_OPT_WITNESS_SCAN_MIN)
SWEEP_MEMBERS = (8, 16, 32, 64, 128, 256, 1024, 16382)
SWEEP_NB = (1, 256)


def synth(shape, nb, size, forms=("lane", "block", "scan")):
    import mpc_dealer as md
    import mpc_bulletproof_amd as m
    prog, v = {"range": lambda: range_program(64, size), "shuffle": lambda: shuffle_program(size), "horner": lambda: horner_program(size)}[shape]()
    chi = (0x1234567,) if prog.nchi else ()
    t0 = time.perf_counter()
    want = prog.evaluate(v, (), chi)
    host_ms = (time.perf_counter() - t0) * 1e3
    gpu = m.BpGpu(0)
    w = gpu.witness_create(*prog.create_args())
    plan = m.lib.witness_plan(*prog.plan_args(), nb)
    chains = m.lib.witness_affine_chains(*prog.plan_args())          # the extended chains: a program without an affine member has its product chains
    longest = max(chains["longest1"], chains["longest2"])
    d_v = gpu.to_device(b"".join(md.mont(x) for x in v) * nb)
    d_chi = gpu.to_device(md.le(chi[0]) * nb) if chi else None
    planes = [gpu.malloc(32 * nb * prog.n) for _ in range(3)]
    timer = Timer(gpu)
    out = {}
    for form in forms:
        if form == "scan" and not longest:       # no chain: route 0 would take the width rule
            continue
        gpu.set_option("witness_route", FORMS[form][0])
        gpu.set_option("witness_scan_min", FORMS[form][1])
        ts = []
        for step in range(WARM + STEPS):
            ms = timer.events(lambda: gpu.r1cs_witness_synthesize_dev(w, nb, 0, *planes, d_v=d_v, d_gadget_challenges=d_chi))
            if step >= WARM:
                ts.append(ms)
        assert gpu.input_flag() == 0
        got = gpu.download(planes[2], 32 * nb * prog.n)
        assert got[-32 * prog.n:] == b"".join(md.mont(x) for x in want[2]), "the device's witness differs from the host's"
        out[form] = ts
    route = plan["route2" if prog.nchi else "route1"]
    cols = "   ".join(f"{form:5s}{fmt(out[form])}" if form in out else f"{form:5s}{'-':>9s}{'':21s}" for form in forms)
    text = (f"{cols}   plan: {('lane', 'block', 'scan')[route - 1]:5s}   levels {plan['levels1'] + plan['levels2']:6d} "
            f"(scan {chains['levels1'] + chains['levels2']:2d})   widest {plan['widest']:5d}   longest chain {longest:6d}   "
            f"host (Python, ONE prover) {host_ms:9.3f}")
    return text, {form: (min(ts), max(ts)) for form, ts in out.items()}


def prove(nb, ks, window_bits):
    import random
    import mpc_dealer as md
    import oracle_lib as o
    import pymodel as pm
    import witness_cases as wc
    import mpc_bulletproof_amd as m
    prog, v = shuffle_program(ks)
    n, mm = prog.n, prog.m
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(b"ShuffleProofTest"))
    pv.pc_gens.commit = lambda val, b: pm.G           # the commitments play no part here: skip the model's scalar multiplications
    vars_ = [pv.commit(x, 1)[1] for x in v]
    pm.shuffle_gadget(pv, vars_[:ks], vars_[ks:])
    pv._create_randomized_constraints()
    rp, kd, ix, cf, _ = md.circuit_rows(pv.constraints, param=True)
    rnd = random.Random(nb)
    rb = lambda cnt: bytes(rnd.getrandbits(8) for _ in range(cnt))      # noqa: E731
    scal = lambda cnt: b"".join(md.mont(rnd.randrange(pm.N)) for _ in range(cnt))      # noqa: E731
    k = (n - 1).bit_length()
    gpu = m.BpGpu(0)
    gens = gpu.gens_create(o.gens("G", 1 << k), o.gens("H", 1 << k), o.generator(), o.generator(), window_bits)
    circ = gpu.circuit_create_param(len(pv.constraints), 1, rp, kd, ix, cf, n, mm)
    w = gpu.witness_create(*prog.create_args())
    bl = [scal(11) for _ in range(nb)]
    d_states, d_v, d_vb = gpu.to_device(rb(32 * nb)), gpu.to_device(b"".join(md.mont(x) for x in v) * nb), gpu.to_device(scal(nb * mm))
    keys = [rb(64) for _ in range(nb)]
    d_bl, d_keys = gpu.to_device(b"".join(bl)), gpu.to_device(b"".join(keys))
    d_bl1, d_bl2 = gpu.to_device(b"".join(b[:96] for b in bl)), gpu.to_device(b"".join(b[96:] for b in bl))
    d_k2 = gpu.to_device(b"".join(x[32:] for x in keys))
    plen = 1 + 14 * 32 + (2 * k + 2) * 32
    d_pts, d_sc, d_wire, d_chi = gpu.malloc(64 * nb * (11 + 2 * k)), gpu.malloc(160 * nb), gpu.malloc(nb * plen), gpu.malloc(32 * nb)
    planes = [gpu.malloc(32 * nb * n) for _ in range(3)]

    def one_call():
        gpu.r1cs_prove_fs2_dev(gens, circ, w, nb, d_states, LABEL, d_bl, d_pts, d_sc, d_v=d_v, d_v_blinding=d_vb, d_vector_keys=d_keys,
                               d_wire=d_wire)
        gpu.sync()

    def two_calls(host_gadget):
        sess = gpu.r1cs_prove_fs2_begin_dev(gens, circ, nb, 0, d_states, LABEL, d_bl1, d_chi=d_chi)
        if host_gadget:
            chi = gpu.download(d_chi, 32 * nb)                         # the round trip: the challenge down, ...
            for k_, plane in enumerate(zip(*(prog.evaluate(v, (), (int.from_bytes(chi[32 * p:32 * p + 32], "little"),)) for p in range(nb)))):
                gpu.upload(planes[k_], b"".join(md.mont(x) for row in plane for x in row))      # ... the witness up
        gpu.r1cs_prove_fs2_finish_dev(gens, circ, sess, *planes, d_bl2, d_pts, d_sc, d_v_blinding=d_vb, d_vector_keys=d_k2, d_wire=d_wire)
        gpu.sync()
    res, wires = {}, {}
    steps = STEPS if nb * n < 20000 else 5
    for name, body in (("one call", one_call), ("two calls + host gadget", lambda: two_calls(True)), ("chains", lambda: two_calls(False))):
        ts = []
        for step in range(WARM + steps):
            t0 = time.perf_counter()
            body()
            if step >= WARM:
                ts.append((time.perf_counter() - t0) * 1e3)
        assert gpu.input_flag() == 0
        res[name], wires[name] = ts, gpu.download(d_wire, nb * plen)
    assert wires["one call"] == wires["two calls + host gadget"], "the one call and the two calls disagree on the proof bytes"
    one, two = statistics.median(res["one call"]), statistics.median(res["two calls + host gadget"])
    return (f"one call {fmt(res['one call'])}   two calls + host gadget (Python) {fmt(res['two calls + host gadget'])}   ratio {two / one:7.2f}   "
            f"chains {fmt(res['chains'])}")


def child(what, args):
    if what == "inv":
        print("RESULT", inv_synth(args[0], int(args[1]), int(args[2])))
    elif what == "divrem":
        print("RESULT", divrem_synth(args[0], int(args[1]), int(args[2]), args[3]))
    elif what == "synth":
        text, spans = synth(args[0], int(args[1]), int(args[2]), tuple(args[3].split(",")))
        print("SPANS", json.dumps(spans))
        print("RESULT", text)
    else:
        print("RESULT", prove(int(args[0]), int(args[1]), int(args[2])))


def scan_min_of(spans, shape):
    """the rule of both thresholds on a sweep's (min, max) spans: the smallest power of two >= 16 from which on the scan's maximum
    lies below the block form's minimum at both batch sizes -> members, or None"""
    def wins(members):
        return all(spans[(shape, nb, members + 2)]["scan"][1] < spans[(shape, nb, members + 2)]["block"][0] for nb in SWEEP_NB)
    powers = [mm for mm in SWEEP_MEMBERS if mm & (mm - 1) == 0 and mm >= 16]
    good = [d for d in powers if all(wins(mm) for mm in SWEEP_MEMBERS if mm >= d)]
    return good[0] if good else None


def scan_min_line(spans):
    """BPGPU_OPT_WITNESS_SCAN_MIN's default from the shuffle sweep"""
    good = [d for d in (scan_min_of(spans, "shuffle"),) if d]
    if not good:
        return "# scan max < block min at both nb from NO measured power of two on: the scan form has missed its purpose"
    return (f"# scan max < block min at both nb from {good[0]} members on (every longer chain of the sweep included): "
            f"BPGPU_OPT_WITNESS_SCAN_MIN defaults to {good[0]}")


def affine_min_line(spans):
    """WIT_AFFINE_MIN from the Horner sweep"""
    d = scan_min_of(spans, "horner")
    if d is None:
        return ("# scan max < block min at both nb from NO measured power of two on: WIT_AFFINE_MIN is set above every chain "
                "(2^25), the plan never scans for an affine chain's sake")
    return f"# scan max < block min at both nb from {d} members on (every longer chain of the sweep included): WIT_AFFINE_MIN = {d}"


def earlier_span(prefix, form):
    """(min, max) of `form` on the last line of profiles/witness_synth.log that starts with `prefix`, and the line"""
    import re
    with open(os.path.join(ROOT, "profiles", "witness_synth.log")) as fh:
        line = [ln for ln in fh.read().splitlines() if ln.startswith(prefix)][-1]
    mm = re.search(form + r"\s+[0-9.]+ \(\s*([0-9.]+)\.\.\s*([0-9.]+)\)", line)
    return (float(mm.group(1)), float(mm.group(2))), line


def runner(title):
    """-> (lines, spans, step): step(text, *child arguments) runs one child and appends its line"""
    spans = {}
    lines = [f"# tools/bench_witness.py {title}  a fresh process per line (limit {STEP_LIMIT} s), {WARM} warm-up + {STEPS} timed steps per route: "
             "median (min..max) ms",
             "# synth: bpgpu_r1cs_witness_synthesize_dev alone, HIP events; host: the same gates of ONE prover on Python integers"]

    def run(*args):
        try:
            out = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] +
                                 [str(a) for a in args], capture_output=True, text=True)
        except OSError as e:
            return f"FAILED to start: {e}", False
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
        if out.returncode != 0 or not got:
            return f"FAILED rc={out.returncode}: {(out.stderr or out.stdout)[-400:]!r}", False
        spans.update({args[1:4]: json.loads(ln[len("SPANS "):]) for ln in out.stdout.splitlines() if ln.startswith("SPANS")})
        return got[0][len("RESULT "):], True

    def step(text, *args):
        res, ok = run(*args)
        lines.append(text + res)
        print(lines[-1])
        sys.stdout.flush()
        return ok
    return lines, spans, step


def affine_main():
    lines, spans, step = runner("affine ")
    lines.append("# the product kernel again (k_witness_scan<false>): each span against the last run of profiles/witness_synth.log +- 8 %")
    ok = True
    for text, nb, k in (("synth   256 x shuffle k = 64       n = 126     ", 256, 64), ("synth   1 x shuffle k = 2^14       n = 32766   ", 1, 1 << 14)):
        ok = ok and step(text, "synth", "shuffle", nb, k, "lane,block,scan")
        if not ok:
            break
        (lo, hi), line = earlier_span(text, "scan")
        now = spans[("shuffle", nb, k)]["scan"]
        inside = lo * 0.92 <= now[0] and now[1] <= hi * 1.08
        lines.append("# earlier " + line[:len(text) + 150].rstrip())
        lines.append(f"# scan now {now[0]:.3f}..{now[1]:.3f} ms against {lo:.3f}..{hi:.3f} ms -8 % / +8 %: {'inside' if inside else 'OUTSIDE'}")
    lines.append("# affine: one Horner pair of k = members + 2 per prover (two affine chains), block form against scan form (k_witness_scan<true>)")
    for members in SWEEP_MEMBERS:
        for nb in SWEEP_NB:
            ok = ok and step(f"affine  {nb:4d} x {members:5d} members   n = {2 * members + 2:5d}   ", "synth", "horner", nb, members + 2, "block,scan")
    if ok:
        lines.append(affine_min_line(spans))
    else:
        lines.append("# a step failed: the steps after it were not started")
    path = os.path.join(ROOT, "profiles", "witness_affine.log")
    with open(path, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[-3:]))
    print("wrote", path)
    return 0 if ok else 1


def inv_main():
    lines, _, step = runner("inv ")
    lines[-1] = ("# inv: bpgpu_r1cs_witness_synthesize_dev alone, HIP events; (a) route 2, one inversion per thread and level; (b) route 1, "
                 "one per gate; (c) the INV gates as INPUT gates fed the pairs, route 2")
    ok = True
    for shape, nb, size in INV_SHAPES:
        text = f"inv     {nb:4d} x {'a chain of' if shape == 'chain' else 'one level of'} {size:4d} INV gates   "
        if ok:
            ok = step(text, "inv", shape, nb, size)
        else:
            lines.append(text + "UNMEASURED")
    if not ok:
        lines.append("# a step failed: the steps after it were not started")
    path = os.path.join(ROOT, "profiles", "witness_inv.log")
    with open(path, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)
    return 0 if ok else 1


def divrem_main():
    lines, _, step = runner("divrem ")
    lines[-1] = ("# divrem: bpgpu_r1cs_witness_synthesize_dev alone, HIP events; (a) route 2 and (b) route 1 on DIVREM gates; (c), (d) the same "
                 "routes with the DIVREM gates as INPUT gates handed the (q, r) pairs; u64: x of 64 bits / y of 33 bits, wide: 252 / 128")
    ok = True
    for shape, nb, size in INV_SHAPES:
        for kind in DIVREM_OPERANDS:
            text = f"divrem  {nb:4d} x {'a chain of' if shape == 'chain' else 'one level of'} {size:4d} DIVREM gates  {kind:4s}   "
            if ok:
                ok = step(text, "divrem", shape, nb, size, kind)
            else:
                lines.append(text + "UNMEASURED")
    if not ok:
        lines.append("# a step failed: the steps after it were not started")
    path = os.path.join(ROOT, "profiles", "witness_divrem.log")
    with open(path, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)
    return 0 if ok else 1


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3:])
    if sys.argv[1:] == ["affine"]:
        return affine_main()
    if sys.argv[1:] == ["inv"]:
        return inv_main()
    if sys.argv[1:] == ["divrem"]:
        return divrem_main()
    lines, spans, step = runner("")
    ok = step("synth   256 x 16 x 64-bit range    n = 1024    ", "synth", "range", 256, 16, "lane,block,scan")
    ok = ok and step("synth   256 x shuffle k = 64       n = 126     ", "synth", "shuffle", 256, 64, "lane,block,scan")
    ok = ok and step("synth   1 x shuffle k = 2^14       n = 32766   ", "synth", "shuffle", 1, 1 << 14, "lane,block,scan")
    lines.append("# sweep: one shuffle of k = members + 2 per prover (two chains), block form against scan form")
    for members in SWEEP_MEMBERS:
        for nb in SWEEP_NB:
            ok = ok and step(f"sweep   {nb:4d} x {members:5d} members   n = {2 * members + 2:5d}   ", "synth", "shuffle", nb, members + 2, "block,scan")
    if ok:
        lines.append(scan_min_line(spans))
    ok = ok and step("synth   4096 x shuffle k = 64      n = 126     ", "synth", "shuffle", 4096, 64, "lane,block,scan")
    lines.append("# prove: wall clock from the first call to the drained stream; chains = begin_dev + finish_dev alone (tools/bench_prove_fs2.py's figure)")
    ok = ok and step("prove   256 x shuffle k = 64       ", "prove", 256, 64, 8)
    ok = ok and step("prove   1 x shuffle k = 2^10       ", "prove", 1, 1 << 10, 8)
    if not ok:
        lines.append("# a step failed: the steps after it were not started")
    path = os.path.join(ROOT, "profiles", "witness_synth.log")
    with open(path, "a") as fh:          # a run is appended: the earlier runs stay, the parent commit's among them
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
