"""The queue policy of libbpgpu.so (include/bpgpu.h: bpgpu_hw_queues) reaches the HIP runtime, and changes no result.

Two fresh child processes, both started with GPU_MAX_HW_QUEUES=4 in their environment: one under the library's default policy
(which raises the 4 to 24 when the library is loaded), the control with BPGPU_HW_QUEUES=0 (the library leaves the 4 alone).  Each
drives 12 single-stream contexts through three bpgpu_r1cs_verify_batch_dev calls each, all 36 issued back to back before the one
synchronisation, with the library's event timing on, and reports

  * the accept bits of every context (256 proofs of the 64-bit range gadget over 8-bit generator tables, one of them tampered;
    256 is the smallest batch whose generator half is walked a proof per lane by default, the form of k_verify_back_q; over 8-bit
    tables the gadget's (generator, window) pairs are more than one chunk and that walk is k_fixed_msm's own launch, so a call is
    seven timed launches), and
  * the largest number of DISTINCT contexts whose timed launches (bpgpu_profile_intervals) are open at one instant.

Packets of one hardware queue run in order, and a launch's interval lies between two marks of its own stream, so under 4 queues at
most 4 contexts can have a launch open at once: the control's bound is a property of the method, not a measurement, and there is no
timing threshold anywhere here.  The default child must show more than 4: its 12 streams have a queue each.
Run with `-m gpu` on an MI355X."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NCTX, CALLS, NB, TAMPERED, N_BITS, WINDOW_BITS = 12, 3, 256, 77, 64, 8


def max_open_contexts(per_ctx):
    """per_ctx[i]: the (start, end) intervals of context i -> the largest number of distinct contexts with an interval open at one
    instant.  An interval that ends at t is closed before one that starts at t opens; a context's own intervals are merged first
    (they follow each other on its one stream, so they never overlap: merging only guards the count against equal stamps)."""
    marks = []
    for iv in per_ctx:
        merged = []
        for a, b in sorted(iv):
            if merged and a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b])
        for a, b in merged:
            if b > a:
                marks += [(a, 1), (b, 0)]
    marks.sort()                                   # at equal times the closing mark (0) sorts before the opening one (1)
    best = cur = 0
    for _, opening in marks:
        cur += 1 if opening else -1
        best = max(best, cur)
    return best


def child():
    sys.path[:0] = [ROOT, HERE]
    import mpc_bulletproof_amd as m
    import bp_helpers as bh
    import oracle_lib as o

    # four proofs from the oracle, the last tampered; the batch is 255 copies of the honest ones around the one tampered proof
    recs, cap = bh.make_range_batch(N_BITS, 4, seed0=7100, tamper={3})
    ins = []
    for proof, com in recs:
        s = o.VerifySession(o.K_RANGE, N_BITS, b"RangeProofTest", [], com, proof, cap)
        k, pts, sc = bh.verify_inputs(proof, com)
        ins.append((pts, sc, s.challenges(), s.rc))
        n1, n2, kk, mm, csr = s.n1, s.n2, s.k, s.m, s.csr()
        s.close()
    assert [rc == 0 for _, _, _, rc in ins] == [True, True, True, False]
    pick = [3 if i == TAMPERED else i % 3 for i in range(NB)]
    pts, sc, ch = (b"".join(ins[j][f] for j in pick) for f in range(3))

    ctxs = [m.BpGpu(0) for _ in range(NCTX)]
    gpu = ctxs[0]
    circ = gpu.circuit_create(*csr, n1 + n2, mm)
    gens = gpu.gens_create(o.gens("G", cap), o.gens("H", cap), o.generator(), o.generator(), WINDOW_BITS)
    d_pts, d_sc, d_ch = gpu.to_device(pts), gpu.to_device(sc), gpu.to_device(ch)
    d_oks = [gpu.malloc(4 * NB) for _ in ctxs]
    for c, d in zip(ctxs, d_oks):                  # one untimed call per context: workspaces, code objects and queues exist
        c.r1cs_verify_batch_dev(gens, circ, NB, n1, kk, d_pts, d_sc, d_ch, d)
    for c in ctxs:
        c.sync()
    for c in ctxs:
        c.profile_enable(True)
    epoch = gpu.profile_epoch()
    for _ in range(CALLS):
        for c, d in zip(ctxs, d_oks):
            c.r1cs_verify_batch_dev(gens, circ, NB, n1, kk, d_pts, d_sc, d_ch, d)
    for c in ctxs:                                 # the one synchronisation, after everything has been issued
        c.sync()
    per_ctx = [[(a, b) for _, a, b in c.profile_intervals(epoch)] for c in ctxs]
    for c in ctxs:
        c.profile_enable(False)
    oks = [[int.from_bytes(raw[4 * i:4 * i + 4], "little") for i in range(NB)] for raw in (c.download(d, 4 * NB) for c, d in zip(ctxs, d_oks))]
    print(json.dumps({"hw_queues": list(m.lib.hw_queues()), "ok": oks, "launches": [len(iv) for iv in per_ctx],
                      "max_open": max_open_contexts(per_ctx), "bad_input": [c.input_flag() for c in ctxs]}))
    for d in [d_pts, d_sc, d_ch] + d_oks:
        gpu.free(d)
    gpu.gens_destroy(gens)
    gpu.circuit_destroy(circ)
    for c in ctxs:
        c.close()


def run_child(own):
    env = {k: v for k, v in os.environ.items() if k != "BPGPU_HW_QUEUES"}
    env.update(GPU_MAX_HW_QUEUES="4", BPGPU_SINGLE_STREAM="1")
    if own is not None:
        env["BPGPU_HW_QUEUES"] = own
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def children():
    default = run_child(None)
    control = run_child("0")               # (started after the first has ended: one process on the GPU at a time)
    print("default policy: hw_queues (inherited, in force) = %s, launches per context = %s, max open contexts = %d"
          % (default["hw_queues"], default["launches"], default["max_open"]))
    print("BPGPU_HW_QUEUES=0: hw_queues (inherited, in force) = %s, launches per context = %s, max open contexts = %d"
          % (control["hw_queues"], control["launches"], control["max_open"]))
    return default, control


def test_interval_sweep_counts_distinct_contexts():
    """the counting itself, on hand-made intervals (no device)"""
    assert max_open_contexts([]) == 0
    assert max_open_contexts([[(0, 1), (1, 2)], [(2, 3)]]) == 1                       # touching intervals do not overlap
    assert max_open_contexts([[(0, 2), (1, 3)], [(4, 5)]]) == 1                       # one context counts once
    assert max_open_contexts([[(0, 2)], [(1, 3)], [(1.5, 1.6)], [(2, 4)]]) == 3
    assert max_open_contexts([[(0, 0)], [(0, 0)]]) == 0                               # empty intervals are never open


def test_policy_changes_no_result(children):
    want = [0 if i == TAMPERED else 1 for i in range(NB)]
    for rep in children:
        assert len(rep["ok"]) == NCTX and all(ok == want for ok in rep["ok"])
        assert rep["bad_input"] == [0] * NCTX
        assert all(n >= CALLS for n in rep["launches"]) and len(set(rep["launches"])) == 1     # every context timed the same launches
    assert children[0]["ok"] == children[1]["ok"]


def test_control_keeps_four_queues(children):
    _, control = children
    assert control["hw_queues"] == [4, 4]
    assert 1 <= control["max_open"] <= 4, control["max_open"]


def test_default_policy_reaches_the_runtime(children):
    default, _ = children
    assert default["hw_queues"] == [4, 24]
    assert default["max_open"] > 4, default["max_open"]


if __name__ == "__main__":
    child()
