#!/usr/bin/env python3
"""bpgpu_r1cs_commit_values_dev beside the route a host had before it.  Writes profiles/commit_values.log (the source of the figures
in DESIGN.md 5.3), one block per shape (nb provers x m commitments, B = B_blinding = the curve generator, window 8):

  256 x 16     the r1cs_prove shape of BASELINE.json (configs[2]);
  4096 x 1     one commitment per prover;
  1 x 32768    the 2^14-shuffle's commitments -- without the transcript: one prover's chain is serial (include/bpgpu.h).

Sides, all under HIP events on the context's stream, in one process:
  one-call     bpgpu_r1cs_commit_values_dev on resident v, v_blinding -> V, V_compressed in HBM, no transcript;
  one-call'    the same call again (the spread between two runs of the same code within an alternation);
  chain        the same with states_in / states_out (not for 1 x 32768);
  two-call     bpgpu_msm_gens_ark(n = 0) on the interleaved (v, v_blinding) rows, then bpgpu_points_compress on the points it returned:
               both host forms, on the same values -- the points travel to the host and back.
ROUNDS alternations after WARM untimed ones; each alternation runs every side once, in an order that rotates.  The bytes of the two
routes are compared at every shape.  median (min..max) ms."""
import ctypes as C
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARM, ROUNDS = 3, 15
SHAPES = ((256, 16, True), (4096, 1, True), (1, 32768, False))


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

    def once(self, call):
        assert self.hip.hipEventRecord(self.ev[0], self.st) == 0
        call()
        assert self.hip.hipEventRecord(self.ev[1], self.st) == 0 and self.hip.hipEventSynchronize(self.ev[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.ev[0], self.ev[1]) == 0
        return ms.value


def shape(gpu, gens, t, nb, m, with_chain, lines):
    import mpc_dealer as md
    import mpc_bulletproof_amd as mm
    lib, N = mm.lib._lib, md.N
    tot = nb * m
    rnd = random.Random(tot)
    v = [md.mont(rnd.randrange(N)) for _ in range(tot)]
    vb = [md.mont(rnd.randrange(N)) for _ in range(tot)]
    rows = b"".join(a + b for a, b in zip(v, vb))
    v, vb = b"".join(v), b"".join(vb)
    init = bytes(rnd.getrandbits(8) for _ in range(32 * nb))
    d_v, d_vb, d_init = gpu.to_device(v), gpu.to_device(vb), gpu.to_device(init)
    d_V, d_Vc, d_so = gpu.malloc(64 * tot), gpu.malloc(32 * tot), gpu.malloc(32 * nb)
    h_V, h_Vc = (C.c_uint8 * (64 * tot))(), (C.c_uint8 * (32 * tot))()      # the two-call route's results, written in place

    def one_call():
        assert lib.bpgpu_r1cs_commit_values_dev(gpu.ctx, gens, nb, m, d_v, d_vb, None, d_V, d_Vc, None) == 0

    def chain():
        assert lib.bpgpu_r1cs_commit_values_dev(gpu.ctx, gens, nb, m, d_v, d_vb, d_init, d_V, d_Vc, d_so) == 0

    def two_call():
        assert lib.bpgpu_msm_gens_ark(gpu.ctx, gens, tot, 0, rows, h_V) == 0
        assert lib.bpgpu_points_compress(gpu.ctx, h_V, tot, h_Vc) == 0

    sides = [("one-call", one_call), ("two-call", two_call), ("one-call'", one_call)] + ([("chain", chain)] if with_chain else [])
    ts = {name: [] for name, _ in sides}
    for r in range(WARM + ROUNDS):
        for i in range(len(sides)):
            name, call = sides[(i + r) % len(sides)]
            ms = t.once(call)
            if r >= WARM:
                ts[name].append(ms)
    assert gpu.input_flag() == 0
    # the two routes' bytes
    two_call()
    one_call()
    V, Vc = gpu.download(d_V, 64 * tot), gpu.download(d_Vc, 32 * tot)
    assert V == bytes(h_V) and Vc == bytes(h_Vc), "the two routes disagree"
    if with_chain:
        chain()
        assert gpu.download(d_V, 64 * tot) == V and gpu.download(d_Vc, 32 * tot) == Vc
        so = gpu.r1cs_commit_values(gens, nb, m, v, vb, init, want_points=False, want_compressed=False)[2]
        assert gpu.download(d_so, 32 * nb) == so
    name = f"{nb}x{m}"
    lines.append(f"# {name}: {tot} commitments; the bytes of the two routes are equal")
    for side, _ in sides:
        lines.append(f"{name:9s} {side:10s} {fmt(ts[side])}")
    a, b, a2 = (statistics.median(ts[s]) for s in ("one-call", "two-call", "one-call'"))
    spread = max(abs(a - a2), max(ts["one-call"]) - min(ts["one-call"]))
    lines.append(f"{name:9s} spread of one-call between its two runs of an alternation: medians {abs(a - a2):.3f} ms apart, range {spread:.3f} ms")
    verdict = "CONFIRMED" if a <= b + spread else "REFUTED"
    lines.append(f"{name:9s} one-call / two-call = {a / b:.3f}: the one call takes no longer than the two-call route beyond that spread -- {verdict}")
    for p in (d_v, d_vb, d_init, d_V, d_Vc, d_so):
        gpu.free(p)


def main():
    import oracle_lib as o
    import mpc_bulletproof_amd as mm
    gpu = mm.BpGpu(0)
    gens = gpu.gens_create(o.gens("G", 2), o.gens("H", 2), o.generator(), o.generator(), 8)
    t = Timer(gpu)
    lines = [f"# tools/bench_commit_values.py   one process, {WARM} warm-up + {ROUNDS} timed alternations per shape, every side once per "
             "alternation in rotating order; HIP events around each side: median (min..max) ms"]
    for nb, m, with_chain in SHAPES:
        shape(gpu, gens, t, nb, m, with_chain, lines)
        print("\n".join(lines[-8:]))
        sys.stdout.flush()
    gpu.gens_destroy(gens)
    gpu.close()
    path = os.path.join(ROOT, "profiles", "commit_values.log")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
