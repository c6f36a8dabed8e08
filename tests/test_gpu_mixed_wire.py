"""Mixed queues of WIRE-format proofs (bpgpu_r1cs_verify_mixed_wire_*): R1CSProof::to_bytes of five circuits -- range gadgets of
two widths, a multi-value range gadget, the example gadget and a two-phase shuffle -- with compressed commitments and transcript
states, decoded, decompressed, challenged and checked in ONE call, against the CPU oracle, against the one-circuit wire entry points
and against the mixed queue on host-decoded operands.  Run with `-m gpu` on an MI355X."""
import json
import os
import random
import sys

import pytest

import bp_helpers as bh
import oracle_lib as o
from test_gpu_mixed_verify import Kind, _ex_values, _group, _rhos, _weighted_sum

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pymodel as pm  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 32
IDENT = bytes(64)
POISON = b"\xff" * 64
SHUFFLE_LABEL = b"shuffle challenge"
COMP_IDENTITY = bytes(31) + b"\x40"
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec.json")) as _f:
    INVALID = [bytes.fromhex(h) for h in json.load(_f)["invalid"]]
OFF_CURVE, BOTH_FLAGS = INVALID[0], INVALID[4]
assert BOTH_FLAGS[31] & 0xC0 == 0xC0


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def gens(gpu):
    g = gpu.gens_create(o.gens("G", CAP), o.gens("H", CAP), o.generator(), o.generator(), 8)
    yield g
    gpu.gens_destroy(g)


@pytest.fixture
def opts(gpu):
    old = {}

    def set_(**kw):
        for k, v in kw.items():
            old.setdefault(k, gpu.get_option(k))
            gpu.set_option(k, v)
    yield set_
    for k, v in old.items():
        gpu.set_option(k, v)


def _wire_of(points, scalars, k, m):
    """operands of bpgpu_r1cs_verify_batch -> (R1CSProof::to_bytes, m x 32 B compressed commitments)"""
    pt = [pm.b2p(points[64 * i:64 * i + 64]) for i in range(11 + m + 2 * k)]
    sc = [pm.b2s(scalars[32 * i:32 * i + 32]) for i in range(5)]
    p = dict(zip(("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2"), pt[:6]))
    p.update(zip(("T_1", "T_3", "T_4", "T_5", "T_6"), pt[6 + m:11 + m]))
    p.update(zip(("t_x", "t_x_blinding", "e_blinding", "a", "b"), sc))
    p["L_vec"], p["R_vec"] = pt[11 + m:11 + m + k], pt[11 + m + k:]
    return pm.r1cs_proof_to_bytes(p), b"".join(pm.point_compress(v) for v in pt[6:6 + m])


class WireKind(Kind):
    """a circuit of the mix with the wire form of every pooled proof beside its decoded operands"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        t = pm.Transcript(self.label)
        if self.param:                                       # the shuffle's preamble before Verifier::new (tests/r1cs.rs:80-81)
            t.append_message(b"dom-sep", b"ShuffleProof")
            t.append_u64(b"k", 6)
        self.init = t.state
        self.head = 11 if self.param else 8                  # compressed points before t_x
        self.plen = 1 + (self.head + 5 + 2 * self.k) * 32
        self.gadget_label = SHUFFLE_LABEL if self.param else None
        for pool in (self.good, self.bad):
            for r in pool:
                r["wire"], r["com"] = _wire_of(r["points"], r["scalars"], self.k, self.m)
                r["init"] = self.init
                assert len(r["wire"]) == self.plen and r["wire"][0] == (1 if self.param else 0)


@pytest.fixture(scope="module")
def mix(gpu):
    kinds = [
        WireKind(gpu, "range8", o.K_RANGE, 8, b"RangeProofTest", 70, lambda r: [r.getrandbits(8)]),
        WireKind(gpu, "range32", o.K_RANGE, 32, b"RangeProofTest", 30, lambda r: [r.getrandbits(32)]),
        WireKind(gpu, "multi3x8", o.K_RANGE_MULTI, 8 | (3 << 16), b"RangeProofTest", 30, lambda r: [r.getrandbits(8) for _ in range(3)]),
        WireKind(gpu, "example", o.K_EXAMPLE, 0, b"R1CSExampleGadget", 30, _ex_values, lambda v: v[-1:]),
        WireKind(gpu, "shuffle6", o.K_SHUFFLE, 6, b"ShuffleProofTest", 20,
                 lambda r: (lambda x: x + r.sample(x, len(x)))([r.getrandbits(40) for _ in range(6)])),
    ]
    assert [kd.k for kd in kinds][:3] == [3, 5, 5] and kinds[4].param and not any(kd.param for kd in kinds[:4])
    yield kinds
    for kd in kinds:
        gpu.circuit_destroy(kd.circ)


def _wgroup(kd, recs, rho):
    return dict(circuit=kd.circ, nb=len(recs), n1=kd.n1, proof_len=kd.plen, proofs=b"".join(r["wire"] for r in recs),
                commitments=b"".join(r["com"] for r in recs), init_states=b"".join(r["init"] for r in recs),
                gadget_label=kd.gadget_label, rho=rho)


def _one_circuit_verdicts(gpu, gens, kd, recs):
    g = _wgroup(kd, recs, b"")
    if kd.param:
        return gpu.r1cs_verify_batch_wire2(gens, kd.circ, len(recs), kd.n1, kd.plen, kd.gadget_label, g["proofs"], g["commitments"],
                                           g["init_states"])
    return gpu.r1cs_verify_batch_wire(gens, kd.circ, len(recs), kd.n1, kd.plen, g["proofs"], g["commitments"], g["init_states"])


def _patch(rec, off, new, ok, field="wire"):
    b = rec[field]
    return dict(rec, **{field: b[:off] + new + b[off + len(new):], "ok": ok})


def _dev_groups(gpu, groups):
    out, allocs = [], []
    for g in groups:
        d = dict(g)
        for f in ("proofs", "commitments", "init_states", "rho"):
            if g.get(f) is not None:
                d[f] = gpu.to_device(g[f] if g["nb"] else b"\0")
                allocs.append(d[f])
        d["ok"] = gpu.to_device(b"\x07" * (4 * max(g["nb"], 1)))
        allocs.append(d["ok"])
        out.append(d)
    return out, allocs


def _ok_of(gpu, d):
    raw = gpu.download(d["ok"], 4 * d["nb"])
    return [int.from_bytes(raw[4 * i:4 * i + 4], "little", signed=True) for i in range(d["nb"])]


def _bad_checks(recs_per_group, batch):
    flat = [r["ok"] for rr in recs_per_group for r in rr]
    return len({i // batch for i, v in enumerate(flat) if not v})


def test_valid_queue(gpu, gens, mix, opts):
    """a valid queue whose runs are 65, 1, 64, 30, 63, 30 and 20 proofs long: as one check (runs of 1, 63, 64 and 65 proofs: the
    edges of the transcript's block table), in checks of 64 and in checks of 16 over three lanes (checks span groups and split
    them) -- every proof accepted, no fallback, and the combined point is the identity"""
    rnd = random.Random(21)
    r8, r32, mu, ex, sh = mix
    plan = [(r8, 65), (r32, 1), (r8, 64), (mu, 30), (r8, 63), (ex, 30), (sh, 20)]
    groups = [_wgroup(kd, kd.pick(range(nb)), b"".join(_rhos(rnd, nb))) for kd, nb in plan]
    for batch, lanes in ((2560, 2), (64, 3), (16, 3)):
        opts(screen_batch=batch, stream_lanes=lanes)
        oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, groups)
        assert oks == [[1] * nb for _, nb in plan], (batch, lanes)
        assert nf == 0, (batch, lanes)
    assert gpu.r1cs_verify_mixed_wire_combined(gens, groups) == IDENT
    assert gpu.input_flag() == 0


def test_screened_equals_the_one_circuit_wire_calls(gpu, gens, mix, opts):
    """random group orders, counts (0 and 1 among them) and tamper sets over several screening batches and lane counts: the verdicts
    equal, group by group, bpgpu_r1cs_verify_batch_wire / _wire2 on that group alone and the oracle's; exactly the checks that hold a
    rejected proof (global proof index // screen_batch: neither the point nor the run cap binds here) take the per-proof path"""
    rnd = random.Random(4242)
    for trial in range(6):
        ng = rnd.randrange(1, 7)
        batch, lanes = rnd.choice((1, 7, 16, 33, 200)), rnd.randrange(1, 5)
        opts(screen_batch=batch, stream_lanes=lanes)
        frac = rnd.choice((0.0, 0.1, 0.4, 1.0))
        groups, recs_all, kinds = [], [], []
        for _ in range(ng):
            kd = rnd.choice(mix)
            nb = rnd.choice((0, 1, 2, 9, 19))
            idx = rnd.sample(range(len(kd.good)), nb)
            recs = kd.pick(idx, {i for i in idx if rnd.random() < frac})
            groups.append(_wgroup(kd, recs, b"".join(_rhos(rnd, nb))))
            recs_all.append(recs)
            kinds.append(kd)
        oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, groups)
        for kd, recs, ok in zip(kinds, recs_all, oks):
            assert ok == [r["ok"] for r in recs], (trial, kd.name, batch, lanes)
            if recs:
                assert _one_circuit_verdicts(gpu, gens, kd, recs) == ok, (trial, kd.name)
        assert nf == _bad_checks(recs_all, batch), (trial, batch, lanes)


def test_crafted_encodings(gpu, gens, mix, opts):
    """one crafted encoding per group: a wrong version byte, an x off the curve in a proof point and in a commitment, both flag bits
    set, the compressed identity as A_I1 (decodes; the transcript's validation rejects it), t_x + n on the wire (the same scalar:
    accepted) and a flipped bit of t_x -- exactly the affected proofs are rejected and exactly their checks fall back"""
    opts(screen_batch=16, stream_lanes=3)
    rnd = random.Random(77)
    r8, r32, mu, ex, sh = mix
    sizes = [40, 30, 30, 30, 20]
    recs = [kd.pick(range(nb)) for kd, nb in zip(mix, sizes)]
    recs[0][3] = _patch(recs[0][3], 0, b"\x01", 0)                                    # version 1 at a one-phase length
    recs[1][2] = _patch(recs[1][2], 1 + 32 * 4, OFF_CURVE, 0)                         # T_3
    recs[2][4] = _patch(recs[2][4], 32 * 1, OFF_CURVE, 0, field="com")               # V_1
    recs[3][1] = _patch(recs[3][1], 1 + 32 * 1, BOTH_FLAGS, 0)                        # A_O1
    recs[4][5] = _patch(recs[4][5], 1, COMP_IDENTITY, 0)                              # A_I1
    off = 1 + 32 * r8.head                                                            # t_x, big-endian
    tx = int.from_bytes(recs[0][20]["wire"][off:off + 32], "big")
    assert tx + o.N < 1 << 256
    recs[0][20] = _patch(recs[0][20], off, (tx + o.N).to_bytes(32, "big"), 1)
    off = 1 + 32 * r32.head
    recs[1][27] = _patch(recs[1][27], off + 31, bytes([recs[1][27]["wire"][off + 31] ^ 4]), 0)
    planted = [(0, 3), (1, 2), (2, 4), (3, 1), (4, 5), (1, 27)]
    want = [[r["ok"] for r in rr] for rr in recs]
    assert sum(v == 0 for w in want for v in w) == len(planted) and want[0][20] == 1
    groups = [_wgroup(kd, rr, b"".join(_rhos(rnd, len(rr)))) for kd, rr in zip(mix, recs)]
    oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, groups)
    assert oks == want
    starts = [sum(sizes[:i]) for i in range(5)]
    assert nf == len({(starts[g] + i) // 16 for g, i in planted}) == _bad_checks(recs, 16)
    for kd, rr, ok in zip(mix, recs, oks):
        assert _one_circuit_verdicts(gpu, gens, kd, rr) == ok, kd.name
    # a zero weight voids its check (every proof of it is re-verified, and accepted)
    rho = _rhos(rnd, 30)
    rho[7] = bytes(32)
    oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, [_wgroup(mu, mu.pick(range(30)), b"".join(rho))])
    assert oks == [[1] * 30] and nf == 1


def test_combined_point(gpu, gens, mix):
    """an all-decodable queue with tampered proofs: the point is the oracle's sum of rho_p * mega_check_p and the one
    bpgpu_r1cs_verify_mixed_combined returns on the host-decoded operands with the oracle's challenges; one undecodable point (or
    an identity at a validated one) turns it into the poison encoding and raises the input flag"""
    rnd = random.Random(31)
    sizes = [12, 7, 9, 6, 5]
    tam = {1: {1, 6}, 3: {0}, 4: {2}}
    recs = [kd.pick(range(nb), tam.get(gi, set())) for gi, (kd, nb) in enumerate(zip(mix, sizes))]
    rhos = [_rhos(rnd, nb) for nb in sizes]
    groups = [_wgroup(kd, rr, b"".join(w)) for kd, rr, w in zip(mix, recs, rhos)]
    got = gpu.r1cs_verify_mixed_wire_combined(gens, groups)
    assert got == _weighted_sum([r for rr in recs for r in rr], [w for ww in rhos for w in ww])
    assert got == gpu.r1cs_verify_mixed_combined(gens, [_group(kd, rr, b"".join(w)) for kd, rr, w in zip(mix, recs, rhos)])
    assert got not in (IDENT, POISON)
    assert gpu.input_flag() == 0
    for gi, i, off, new, field in ((2, 3, 1 + 32 * 2, OFF_CURVE, "wire"), (0, 5, 0, OFF_CURVE, "com"), (4, 1, 1, COMP_IDENTITY, "wire")):
        rr = [list(x) for x in recs]
        rr[gi][i] = _patch(rr[gi][i], off, new, 0, field=field)
        bad = [_wgroup(kd, x, b"".join(w)) for kd, x, w in zip(mix, rr, rhos)]
        assert gpu.r1cs_verify_mixed_wire_combined(gens, bad) == POISON, (gi, i)
        assert gpu.input_flag() == 1
    # no proofs at all: the identity
    assert gpu.r1cs_verify_mixed_wire_combined(gens, []) == IDENT
    assert gpu.r1cs_verify_mixed_wire_combined(gens, [_wgroup(mix[1], [], b"")]) == IDENT
    oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, [_wgroup(mix[4], [], b""), _wgroup(mix[0], [], b"")])
    assert oks == [[], []] and nf == 0


def test_device_forms(gpu, gens, mix, opts):
    """operands and verdicts in HBM: the host forms' verdicts after sync(), the same combined point; and two groups that share
    one circuit handle under different transcript states -- a proof made under another label passes in the group that carries
    its state and fails in the other"""
    opts(screen_batch=16, stream_lanes=3)
    rnd = random.Random(58)
    r8 = mix[0]
    other = []
    for i in range(3):
        rc, proof, com = o.r1cs_prove(o.K_RANGE, 8, b"AnotherLabel", [17 + i], 5000 + i, CAP)
        assert rc == 0
        k, pts, sc = bh.verify_inputs(proof, com)
        wire, cc = _wire_of(pts, sc, k, 1)
        other.append(dict(wire=wire, com=cc))
    st_a, st_b = r8.init, pm.Transcript(b"AnotherLabel").state
    assert st_a != st_b
    sizes = [9, 4, 0, 6, 3]
    recs = [kd.pick(range(nb), {1} if kd.name == "range32" else set()) for kd, nb in zip(mix, sizes)]
    mixed_a = [dict(r, init=st_a) for r in r8.pick(range(4))] + [dict(other[0], init=st_a, ok=0), dict(other[1], init=st_a, ok=0)]
    mixed_b = [dict(x, init=st_b, ok=1) for x in other] + [dict(r8.good[5], init=st_b, ok=0)]
    kinds = list(mix) + [r8, r8]
    recs += [mixed_a, mixed_b]
    groups = [_wgroup(kd, rr, b"".join(_rhos(rnd, len(rr)))) for kd, rr in zip(kinds, recs)]
    want = [[r["ok"] for r in rr] for rr in recs]
    oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, groups)
    assert oks == want and nf == _bad_checks(recs, 16)
    point = gpu.r1cs_verify_mixed_wire_combined(gens, groups)
    assert point not in (IDENT, POISON)
    dg, allocs = _dev_groups(gpu, groups)
    dout = gpu.malloc(64)
    try:
        for rep in range(2):                                  # (twice: the second call reuses the lanes' workspaces and the staging)
            assert gpu.r1cs_verify_mixed_wire_screened_dev(gens, dg) == nf
        gpu.sync()
        assert [_ok_of(gpu, d) for d in dg] == want
        gpu.r1cs_verify_mixed_wire_combined_dev(gens, dg, dout)
        gpu.sync()
        assert gpu.download(dout, 64) == point
    finally:
        gpu.free(dout)
        for a in allocs:
            gpu.free(a)


def test_shape_errors_fail_before_anything_runs(gpu, gens, mix):
    import mpc_bulletproof_amd as m
    E = m.lib
    rnd = random.Random(3)
    r8, r32, sh = mix[0], mix[1], mix[4]
    small = gpu.gens_create(o.gens("G", 8), o.gens("H", 8), o.generator(), o.generator(), 8)
    # the shuffle's rows as a circuit with TWO gadget challenges (a third, empty block of rows)
    rp, kd_, ix, cf = sh.csr
    rows0, rows1 = [[] for _ in range(sh.q)], [[] for _ in range(sh.q)]
    for r in range(sh.q):
        for t in range(rp[r], rp[r + 1]):
            (rows1 if kd_[t] == 4 else rows0)[r].append((4, 0, (o.N - 1).to_bytes(32, "little")) if kd_[t] == 4 else (kd_[t], ix[t], cf[32 * t:32 * t + 32]))
    prp, pkd, pix, pcf = [0], [], [], b""
    for row in rows0 + rows1 + [[] for _ in range(sh.q)]:
        for a, b, c in row:
            pkd.append(a)
            pix.append(b)
            pcf += c
        prp.append(len(pkd))
    two_chi = gpu.circuit_create_param(sh.q, 2, prp, pkd, pix, pcf, sh.n, sh.m)
    try:
        def grp(kd, nb, **over):
            return dict(_wgroup(kd, kd.pick(range(nb)), b"".join(_rhos(rnd, nb))), **over)
        good = grp(r8, 4)
        cases = [
            (gens, [good, grp(r8, 2, proof_len=r8.plen + 1)], E.E_LEN),              # no proof has this length
            (gens, [good, grp(r8, 2, proof_len=r8.plen + 32)], E.E_LEN),
            (gens, [good, grp(r8, 2, circuit=r32.circ)], E.E_LEN),                   # 2^k from the length is not the circuit's padded n
            (gens, [good, grp(r8, 2, n1=r8.n + 1)], E.E_LEN),
            (small, [good, grp(r32, 3)], E.E_GENS),
            (gens, [good, grp(r8, 2, rho=None)], E.E_ARG),
            (gens, [good, grp(r8, 2, init_states=None)], E.E_ARG),
            (gens, [good, grp(r8, 2, commitments=None)], E.E_ARG),
            (gens, [good, grp(sh, 2, gadget_label=None)], E.E_ARG),
            (gens, [good, grp(r8, 2, gadget_label=SHUFFLE_LABEL)], E.E_ARG),
            (gens, [good, grp(sh, 2, circuit=two_chi)], E.E_ARG),
        ]
        for ci, (gg, groups, code) in enumerate(cases):
            dg, allocs = _dev_groups(gpu, groups)
            try:
                for call in (lambda: gpu.r1cs_verify_mixed_wire_screened_dev(gg, dg), lambda: gpu.r1cs_verify_mixed_wire_screened(gg, groups),
                             lambda: gpu.r1cs_verify_mixed_wire_combined_dev(gg, dg, dg[0]["ok"]),
                             lambda: gpu.r1cs_verify_mixed_wire_combined(gg, groups)):
                    with pytest.raises(E.BpGpuError) as e:
                        call()
                    assert e.value.code == code, ci
                gpu.sync()
                for d in dg:                                            # nothing launched: no verdict (and no point) written
                    assert gpu.download(d["ok"], 4 * d["nb"]) == b"\x07" * (4 * d["nb"]), ci
            finally:
                for a in allocs:
                    gpu.free(a)
        for call in (gpu.r1cs_verify_mixed_wire_combined, gpu.r1cs_verify_mixed_wire_screened):
            with pytest.raises(E.BpGpuError) as e:
                call(gens, [good] * (E.MIXED_MAX_GROUPS + 1))
            assert e.value.code == E.E_ARG
        # the context is fine afterwards
        oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, [good])
        assert oks == [[1] * 4] and nf == 0
    finally:
        gpu.circuit_destroy(two_chi)
        gpu.gens_destroy(small)


def test_more_groups_than_one_check_takes(gpu, gens, mix, opts):
    """20 small groups of wire bytes, more than the 16 group runs one check holds (BPGPU_MIXED_MAX_SEGMENTS): the combined call adds
    up the points of two checks, each behind its own ragged front, and equals the decoded queue's call on the host-decoded operands
    of the same records and weights (the identity on valid proofs; an off-curve point in the last group poisons the sum), and the
    screened call closes a check after 16 groups -- its verdicts equal the oracle's and exactly the check that holds the tampered
    proof falls back"""
    import mpc_bulletproof_amd as m
    assert m.lib.MIXED_MAX_SEGMENTS == 16
    rnd = random.Random(2020)
    ng = 20
    kinds = [mix[i % 5] for i in range(ng)]
    nxt = {kd.name: 0 for kd in mix}

    def take(kd, nb):
        idx = list(range(nxt[kd.name], nxt[kd.name] + nb))
        nxt[kd.name] += nb
        return idx
    idxs = [take(kd, 1 + i % 2) for i, kd in enumerate(kinds)]
    rhos = [_rhos(rnd, len(ix)) for ix in idxs]

    def queues(recs):
        return ([_wgroup(kd, r, b"".join(w)) for kd, r, w in zip(kinds, recs, rhos)],
                [_group(kd, r, b"".join(w)) for kd, r, w in zip(kinds, recs, rhos)])
    valid = [kd.pick(ix) for kd, ix in zip(kinds, idxs)]
    wire, decoded = queues(valid)
    got = gpu.r1cs_verify_mixed_wire_combined(gens, wire)
    assert got == gpu.r1cs_verify_mixed_combined(gens, decoded)
    assert got == IDENT
    assert gpu.input_flag() == 0
    # one tampered proof in group 18: the second check
    recs = [kd.pick(ix, {ix[0]} if g == 18 else set()) for g, (kd, ix) in enumerate(zip(kinds, idxs))]
    assert recs[18][0]["ok"] == 0
    wire, decoded = queues(recs)
    got = gpu.r1cs_verify_mixed_wire_combined(gens, wire)
    assert got == gpu.r1cs_verify_mixed_combined(gens, decoded)
    assert got not in (IDENT, POISON)
    assert gpu.input_flag() == 0
    opts(screen_batch=2560, stream_lanes=3)
    oks, nf = gpu.r1cs_verify_mixed_wire_screened(gens, wire)
    assert oks == [[x["ok"] for x in r] for r in recs]
    assert nf == 1
    # an off-curve point in group 19
    recs[19] = [_patch(recs[19][0], 1 + 32 * 2, OFF_CURVE, 0)] + recs[19][1:]
    wire, _ = queues(recs)
    assert gpu.r1cs_verify_mixed_wire_combined(gens, wire) == POISON
    assert gpu.input_flag() == 1
