#!/usr/bin/env python3
"""The two-party witness sessions (bpgpu_mpc_witness_mask / _combine, include/bpgpu.h): the device part of ONE _mask + _combine pair,
i.e. of one dependency level of one party -- the operands' conversion, the level's launch and the results' conversion, as the
library's own HIP events time them (profiling kind 22; the host's copies and waits around them are not in the figure).  Appends a run
to profiles/mpc_witness.log.  Shapes: 256 proofs of a one-level program of 1 024 INPUT gates (the range gadget on shares), 256 proofs
of the 64-shuffle (63 levels of 2 gates: a pair per level, the median over all pairs of a session), one proof of a 300-gate-wide
level.  The operands are random shares: the timing does not depend on their values, and nothing is opened (`opened` is random too).

A fresh process per line under its own time limit; WARM untimed sessions, then STEPS timed ones, medians (min..max) in ms."""
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

WARM, STEPS = 2, 10
STEP_LIMIT = 300          # seconds per child process
KIND = "prove_fs_links"   # kind 22


def fmt(ts):
    return f"{statistics.median(ts):9.3f} ({min(ts):8.3f}..{max(ts):9.3f})"


def program(shape):
    import witness_cases as wc
    if shape == "inputs":
        prog = wc.Program(0)
        for _ in range(1024):
            prog.input()
        return prog
    if shape == "shuffle":
        prog = wc.Program(128, nchi=1)
        prog.end_phase1()
        wc._shuffle_gates(prog, 64, 0)
        return prog
    prog = wc.Program(4)
    for i in range(300):
        prog.mul([(wc.V, i % 4, 1), (wc.ONE, 0, i)], [(wc.V, (i + 1) % 4, 1)])
    return prog


def child(shape, nb):
    import mpc_dealer as md
    import mpc_bulletproof_amd as m
    prog = program(shape)
    rnd = random.Random(nb)
    scal = lambda cnt: b"".join(md.mont(rnd.randrange(md.N)) for _ in range(cnt)) or None      # noqa: E731
    levels = m.lib.witness_gate_levels(*prog.plan_args())
    widths = [levels.count(l) for l in range(max(levels) + 1)]
    gpu = m.BpGpu(0)
    w = gpu.witness_create(*prog.create_args())
    v, inputs = scal(nb * 3 * prog.m), scal(nb * 3 * 2 * prog.ninp)
    chi = b"".join(md.le(rnd.randrange(md.N)) for _ in range(nb * prog.nchi)) or None
    phase = 2 if prog.nchi else 0
    planes = [bytes(32 * nb * 3 * prog.n)] * 3 if phase == 2 else [None] * 3
    trips = {g: scal(nb * 9 * g) for g in set(widths)}
    opened = {g: scal(nb * 2 * g) for g in set(widths)}
    gpu.profile_enable(True)
    gpu.profile_select([KIND])
    pairs = []
    for step in range(WARM + STEPS):
        s = gpu.mpc_witness_begin(w, nb, phase, v, inputs, chi, *planes)
        gpu.profile_read()
        for g in widths:
            assert gpu.mpc_witness_level_len(s) == g
            gpu.mpc_witness_mask(s, nb, trips[g])
            gpu.mpc_witness_combine(s, opened[g])
            ms, cnt = gpu.profile_read()[KIND]
            assert cnt == 2
            if step >= WARM:
                pairs.append(ms)
        gpu.mpc_witness_finish(s, nb, prog.n)
        gpu.mpc_witness_destroy(s)
    print(f"RESULT mask + combine {fmt(pairs)}   levels {len(widths):3d}   widest {max(widths):5d}   pairs timed {len(pairs):4d}")


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]))
    lines = [f"# tools/bench_mpc_witness.py  a fresh process per line (limit {STEP_LIMIT} s), {WARM} warm-up + {STEPS} timed sessions: "
             "median (min..max) ms of ONE _mask + _combine pair of ONE party, device part (profiling kind 22)"]
    ok = True
    for text, shape, nb in (("pair    256 x 1024 INPUT gates     n = 1024   ", "inputs", 256), ("pair    256 x shuffle k = 64       n = 126    ", "shuffle", 256),
                            ("pair    1 x 300-gate level         n = 300    ", "wide", 1)):
        if not ok:
            break
        out = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--child", shape, str(nb)],
                             capture_output=True, text=True)
        got = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
        ok = out.returncode == 0 and bool(got)
        lines.append(text + (got[0][len("RESULT "):] if ok else f"FAILED rc={out.returncode}: {(out.stderr or out.stdout)[-400:]!r}"))
        print(lines[-1])
        sys.stdout.flush()
    if not ok:
        lines.append("# a step failed: the steps after it were not started")
    path = os.path.join(ROOT, "profiles", "mpc_witness.log")
    with open(path, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
