"""Mixed queues: proofs of several circuits -- range gadgets of two widths, a multi-value range gadget, the example gadget and a
two-phase shuffle -- in ONE combined or screened call (bpgpu_r1cs_verify_mixed_*), against the CPU oracle and against the
one-circuit entry points.  Run with `-m gpu` on an MI355X."""
import random

import pytest

import bp_helpers as bh
import oracle_lib as o

pytestmark = pytest.mark.gpu
CAP = 32          # the largest padded n of the mix (32-bit range, 3 x 8-bit range); the generators are a prefix chain
IDENT = bytes(64)
POISON = b"\xff" * 64


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


def _tamper(proof, i):
    bad = bytearray(proof)
    bad[8 + 11 * 64 + (i % 3) * 32] ^= 1 + (i % 7)      # a bit of t_x / t_x_blinding / e_blinding
    return bytes(bad)


class Kind:
    """one circuit of the mix: a pool of valid proofs and of the same proofs tampered, as operands of bpgpu_r1cs_verify_batch"""

    def __init__(self, gpu, name, kind, param, label, count, values, verify_values=lambda v: []):
        self.name, self.label = name, label
        self.good, self.bad = [], []
        rnd = random.Random(sum(name.encode()))
        for i in range(count):
            vals = values(rnd)
            rc, proof, com = o.r1cs_prove(kind, param, label, vals, 900 + 31 * i, CAP)
            assert rc == 0, name
            for dst, pr in ((self.good, proof), (self.bad, _tamper(proof, i))):
                s = o.VerifySession(kind, param, label, verify_values(vals), com, pr, CAP)
                k, pts, sc = bh.verify_inputs(pr, com)
                chi = b""
                if kind == o.K_SHUFFLE:                  # the gadget challenge z: the oracle's rows carry -z as the `One` coefficients
                    _, kd, _, cf = s.csr()
                    ones = {cf[32 * t:32 * t + 32] for t in range(len(kd)) if kd[t] == 4}
                    assert len(ones) == 1
                    chi = o.s2b((o.N - o.b2s(ones.pop())) % o.N)
                dst.append(dict(points=pts, scalars=sc, challenges=s.challenges(), chi=chi, ok=1 if s.rc == 0 else 0,
                                mega=s.mega_check()))
                if i == 0 and dst is self.good:
                    self.n1, self.k, self.m, self.n = s.n1, s.k, s.m, s.n1 + s.n2
                    self.csr, self.q = s.csr(), s.q
                s.close()
            assert self.good[-1]["ok"] == 1 and self.bad[-1]["ok"] == 0, name
        self.nvar = 11 + self.m + 2 * self.k
        self.param = kind == o.K_SHUFFLE
        if self.param:                                   # parametric CSR: every `One` term of the shuffle rows is chi * (-1)
            rp, kd, ix, cf = self.csr
            rows0, rows1 = [[] for _ in range(self.q)], [[] for _ in range(self.q)]
            for r in range(self.q):
                for t in range(rp[r], rp[r + 1]):
                    if kd[t] == 4:
                        rows1[r].append((4, 0, (o.N - 1).to_bytes(32, "little")))
                    else:
                        rows0[r].append((kd[t], ix[t], cf[32 * t:32 * t + 32]))
            prp, pkd, pix, pcf = [0], [], [], b""
            for row in rows0 + rows1:
                for a, b, c in row:
                    pkd.append(a)
                    pix.append(b)
                    pcf += c
                prp.append(len(pkd))
            self.circ = gpu.circuit_create_param(self.q, 1, prp, pkd, pix, pcf, self.n, self.m)
        else:
            self.circ = gpu.circuit_create(*self.csr, self.n, self.m)

    def pick(self, idx, tamper=()):
        return [self.bad[i] if i in tamper else self.good[i] for i in idx]


def _ex_values(rnd):
    """(a1 + a2)(b1 + b2) = c1 + c2 with the public c2 = 9: the public input is part of the circuit, so it is one for all proofs"""
    a, b, c, d = (rnd.randrange(2, 50) for _ in range(4))
    return [a, b, c, d, (a + b) * (c + d) - 9, 9]


@pytest.fixture(scope="module")
def mix(gpu):
    kinds = [
        Kind(gpu, "range8", o.K_RANGE, 8, b"RangeProofTest", 40, lambda r: [r.getrandbits(8)]),
        Kind(gpu, "range32", o.K_RANGE, 32, b"RangeProofTest", 30, lambda r: [r.getrandbits(32)]),
        Kind(gpu, "multi3x8", o.K_RANGE_MULTI, 8 | (3 << 16), b"RangeProofTest", 30, lambda r: [r.getrandbits(8) for _ in range(3)]),
        Kind(gpu, "example", o.K_EXAMPLE, 0, b"R1CSExampleGadget", 30, _ex_values, lambda v: v[-1:]),
        Kind(gpu, "shuffle6", o.K_SHUFFLE, 6, b"ShuffleProofTest", 20,
             lambda r: (lambda x: x + r.sample(x, len(x)))([r.getrandbits(40) for _ in range(6)])),
    ]
    assert [kd.k for kd in kinds][:3] == [3, 5, 5] and kinds[4].param and not any(kd.param for kd in kinds[:4])
    yield kinds
    for kd in kinds:
        gpu.circuit_destroy(kd.circ)


def _group(kd, recs, rho):
    return dict(circuit=kd.circ, nb=len(recs), n1=kd.n1, k=kd.k, points=b"".join(r["points"] for r in recs),
                scalars=b"".join(r["scalars"] for r in recs), challenges=b"".join(r["challenges"] for r in recs),
                gadget_challenges=b"".join(r["chi"] for r in recs) if kd.param else None, rho=rho)


def _rhos(rnd, n):
    return [o.s2b(rnd.randrange(1, o.N)) for _ in range(n)]


def _weighted_sum(recs, rhos):
    acc = IDENT
    for r, w in zip(recs, rhos):
        acc = o.point_add(acc, o.point_mul(w, r["mega"]))
    return acc


def _per_group_verdicts(gpu, gens, kd, recs):
    g = _group(kd, recs, b"")
    if kd.param:
        ok, _, _ = gpu.r1cs_verify_batch_param(gens, kd.circ, len(recs), kd.n1, kd.k, kd.m, g["points"], g["scalars"], g["challenges"],
                                               g["gadget_challenges"], False, False)
    else:
        ok, _, _ = gpu.r1cs_verify_batch(gens, kd.circ, len(recs), kd.n1, kd.k, kd.m, g["points"], g["scalars"], g["challenges"], False, False)
    return list(ok)


def _off_curve(rec):
    pts = rec["points"]
    y = (int.from_bytes(pts[64 + 32:128], "little") + 1) % (1 << 251)     # second point: y := y + 1 leaves the curve
    return dict(rec, points=pts[:96] + y.to_bytes(32, "little") + pts[128:], ok=0)


def test_combined_point_equals_the_oracle(gpu, gens, mix):
    """partial_xy = sum_p rho_p * mega_check_p over all five groups, byte for byte; the identity exactly when nothing is tampered"""
    rnd = random.Random(11)
    sizes = [12, 7, 9, 6, 5]
    for tampered in (False, True):
        groups, all_recs, all_rho = [], [], []
        for kd, nb in zip(mix, sizes):
            tam = {1, nb - 1} if tampered and kd.name in ("range32", "shuffle6") else ({0} if tampered and kd.name == "example" else set())
            recs = kd.pick(range(nb), tam)
            rho = _rhos(rnd, nb)
            groups.append(_group(kd, recs, b"".join(rho)))
            all_recs += recs
            all_rho += rho
        got = gpu.r1cs_verify_mixed_combined(gens, groups)
        want = _weighted_sum(all_recs, all_rho)
        assert got == want, tampered
        assert (got == IDENT) == (not tampered)
    # the shuffle group alone (a parametric circuit in the combined check), and a malformed point: the poison encoding
    kd = mix[4]
    recs = kd.pick(range(6), {2})
    rho = _rhos(rnd, 6)
    assert gpu.r1cs_verify_mixed_combined(gens, [_group(kd, recs, b"".join(rho))]) == _weighted_sum(recs, rho)
    recs = [_off_curve(r) if i == 3 else r for i, r in enumerate(mix[0].pick(range(8)))]
    assert gpu.r1cs_verify_mixed_combined(gens, [_group(mix[0], recs, b"".join(_rhos(rnd, 8)))]) == POISON
    assert gpu.input_flag() == 1
    # no proofs at all: the identity
    assert gpu.r1cs_verify_mixed_combined(gens, []) == IDENT
    assert gpu.r1cs_verify_mixed_combined(gens, [_group(mix[1], [], b"")]) == IDENT


@pytest.mark.parametrize("nb", [5, 24])      # 5 x 18 proof points: the generic MSMs; 24 x 18: the one-instance bucket pipeline
def test_one_group_equals_the_one_circuit_combined_call(gpu, gens, mix, nb):
    kd = mix[0]
    rnd = random.Random(nb)
    for tam in (set(), {1}):
        recs = kd.pick(range(nb), tam)
        rho = b"".join(_rhos(rnd, nb))
        g = _group(kd, recs, rho)
        one = gpu.r1cs_verify_combined(gens, kd.circ, nb, kd.n1, kd.k, kd.m, g["points"], g["scalars"], g["challenges"], rho)
        assert gpu.r1cs_verify_mixed_combined(gens, [g]) == one
        assert (one == IDENT) == (not tam)
        # the same proofs split over two groups of the same circuit handle: the same point
        h = nb // 2
        g1, g2 = _group(kd, recs[:h], rho[:32 * h]), _group(kd, recs[h:], rho[32 * h:])
        assert gpu.r1cs_verify_mixed_combined(gens, [g1, g2]) == one


def _dev_groups(gpu, groups):
    """device copies of the groups' operands (and an ok array each); -> (device groups, allocations)"""
    out, allocs = [], []
    for g in groups:
        d = dict(g)
        for f in ("points", "scalars", "challenges", "gadget_challenges", "rho"):
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


def test_screened_verdicts_equal_the_oracle(gpu, gens, mix, opts):
    """~150 proofs over five groups, checks of 16 proofs over three lanes (checks span and split groups).  All valid: no fallback.
    Then tampered proofs in two groups (one of them the shuffle), an off-curve point in a third and a zero weight in a fourth:
    the verdicts equal the oracle's proof by proof, and exactly the checks holding one of them take the per-proof path."""
    opts(screen_batch=16, stream_lanes=3)
    rnd = random.Random(5)
    sizes = [40, 30, 30, 30, 20]
    rho = [_rhos(rnd, nb) for nb in sizes]
    groups = [_group(kd, kd.pick(range(nb)), b"".join(r)) for kd, nb, r in zip(mix, sizes, rho)]
    for rep in range(2):
        oks, nf = gpu.r1cs_verify_mixed_screened(gens, groups)
        assert oks == [[1] * nb for nb in sizes] and nf == 0, rep
    tam = {0: {5}, 4: {3, 17}}
    recs = [kd.pick(range(nb), tam.get(gi, set())) for gi, (kd, nb) in enumerate(zip(mix, sizes))]
    recs[1][10] = _off_curve(recs[1][10])
    rho[2][7] = bytes(32)
    groups = [_group(kd, r, b"".join(w)) for kd, r, w in zip(mix, recs, rho)]
    want = [[r["ok"] for r in rr] for rr in recs]
    assert want[2] == [1] * 30 and want[1][10] == 0 and want[4][3] == want[4][17] == want[0][5] == 0
    starts = [sum(sizes[:i]) for i in range(5)]
    planted = [(0, 5), (4, 3), (4, 17), (1, 10), (2, 7)]
    oks, nf = gpu.r1cs_verify_mixed_screened(gens, groups)
    assert oks == want
    assert nf == len({(starts[g] + i) // 16 for g, i in planted})
    for kd, rr, ok in zip(mix, recs, oks):
        assert _per_group_verdicts(gpu, gens, kd, rr) == ok, kd.name
    # device form: the same verdicts and fallback count
    dg, allocs = _dev_groups(gpu, groups)
    try:
        assert gpu.r1cs_verify_mixed_screened_dev(gens, dg) == nf
        gpu.sync()
        assert [_ok_of(gpu, d) for d in dg] == want
    finally:
        for a in allocs:
            gpu.free(a)


def test_screened_random_shapes(gpu, gens, mix, opts):
    """random group counts (1-6), empty groups, the same circuit in two groups, screening batches that divide nothing, one to five
    lanes, tamper sets from none to all: the verdicts always equal per-group bpgpu_r1cs_verify_batch(_param)"""
    rnd = random.Random(777)
    for trial in range(8):
        ng = rnd.randrange(1, 7)
        batch, lanes = rnd.choice((1, 5, 13, 33, 64, 200)), rnd.randrange(1, 6)
        opts(screen_batch=batch, stream_lanes=lanes)
        frac = rnd.choice((0.0, 0.05, 0.3, 1.0))
        groups, recs_all, kinds = [], [], []
        for _ in range(ng):
            kd = rnd.choice(mix)
            nb = rnd.choice((0, 1, 3, 8, 17))
            idx = rnd.sample(range(len(kd.good)), nb)
            recs = kd.pick(idx, {i for i in idx if rnd.random() < frac})
            groups.append(_group(kd, recs, b"".join(_rhos(rnd, nb))))
            recs_all.append(recs)
            kinds.append(kd)
        oks, nf = gpu.r1cs_verify_mixed_screened(gens, groups)
        for kd, recs, ok in zip(kinds, recs_all, oks):
            want = [r["ok"] for r in recs]
            assert ok == want, (trial, kd.name, batch, lanes)
            if recs:
                assert _per_group_verdicts(gpu, gens, kd, recs) == want
        flat = [r["ok"] for rr in recs_all for r in rr]
        bad_checks = {i // batch for i, v in enumerate(flat) if not v}
        assert nf == len(bad_checks), (trial, batch, lanes)


def test_host_and_device_forms_agree(gpu, gens, mix):
    rnd = random.Random(99)
    sizes = [9, 4, 0, 6, 3]
    groups = [_group(kd, kd.pick(range(nb), {1} if kd.name == "range32" else set()), b"".join(_rhos(rnd, nb))) for kd, nb in zip(mix, sizes)]
    want = gpu.r1cs_verify_mixed_combined(gens, groups)
    dg, allocs = _dev_groups(gpu, groups)
    dout = gpu.malloc(64)
    try:
        gpu.r1cs_verify_mixed_combined_dev(gens, dg, dout)
        gpu.sync()
        assert gpu.download(dout, 64) == want != IDENT
        oks, nf = gpu.r1cs_verify_mixed_screened(gens, groups)
        assert gpu.r1cs_verify_mixed_screened_dev(gens, dg) == nf
        gpu.sync()
        assert [_ok_of(gpu, d) for d in dg] == oks
        assert oks[1] == [1, 0, 1, 1] and oks[2] == []
    finally:
        gpu.free(dout)
        for a in allocs:
            gpu.free(a)


def test_argument_errors_fail_before_anything_runs(gpu, gens, mix):
    import mpc_bulletproof_amd as m
    rnd = random.Random(3)
    kd8, kd32, sh = mix[0], mix[1], mix[4]
    small = gpu.gens_create(o.gens("G", 8), o.gens("H", 8), o.generator(), o.generator(), 8)
    try:
        good = _group(kd8, kd8.pick(range(4)), b"".join(_rhos(rnd, 4)))
        cases = [
            (small, [good, _group(kd32, kd32.pick(range(3)), b"".join(_rhos(rnd, 3)))], m.lib.E_GENS),
            (gens, [good, dict(_group(kd8, kd8.pick(range(2)), b"".join(_rhos(rnd, 2))), k=32)], m.lib.E_LEN),
            (gens, [good, dict(_group(sh, sh.pick(range(2)), b"".join(_rhos(rnd, 2))), gadget_challenges=None)], m.lib.E_ARG),
        ]
        for gg, groups, code in cases:
            dg, allocs = _dev_groups(gpu, groups)
            try:
                for call in (lambda: gpu.r1cs_verify_mixed_screened_dev(gg, dg), lambda: gpu.r1cs_verify_mixed_combined_dev(gg, dg, dg[0]["ok"]),
                             lambda: gpu.r1cs_verify_mixed_screened(gg, groups)):
                    with pytest.raises(m.lib.BpGpuError) as e:
                        call()
                    assert e.value.code == code
                gpu.sync()
                for d in dg:                                            # no verdict written
                    assert gpu.download(d["ok"], 4 * d["nb"]) == b"\x07" * (4 * d["nb"])
            finally:
                for a in allocs:
                    gpu.free(a)
        with pytest.raises(m.lib.BpGpuError) as e:
            gpu.r1cs_verify_mixed_combined(gens, [good] * 65)
        assert e.value.code == m.lib.E_ARG
        # the context is fine afterwards
        oks, nf = gpu.r1cs_verify_mixed_screened(gens, [good])
        assert oks == [[1] * 4] and nf == 0
    finally:
        gpu.gens_destroy(small)


def test_more_groups_than_one_check_takes(gpu, gens, mix, opts):
    """40 small groups, more than the 16 group runs one check holds (BPGPU_MIXED_MAX_SEGMENTS): the combined call adds up the
    points of three checks and equals the oracle (a malformed point in the last check poisons the sum), and the screened call
    closes a check every 16 groups -- its verdicts equal the oracle's and exactly the checks holding a bad proof fall back"""
    import mpc_bulletproof_amd as m
    assert m.lib.MIXED_MAX_SEGMENTS == 16
    rnd = random.Random(4040)
    ng = 40
    kinds = [mix[i % 5] for i in range(ng)]
    nxt = {kd.name: 0 for kd in mix}

    def take(kd, nb):
        idx = [(nxt[kd.name] + j) % len(kd.good) for j in range(nb)]
        nxt[kd.name] += nb
        return idx
    idxs = [take(kd, 1 + i % 3) for i, kd in enumerate(kinds)]
    bad_groups = {5: 0, 35: 1}                     # group -> its tampered proof: checks 0 and 2
    for tampered in (False, True):
        recs = [kd.pick(ix, {ix[bad_groups[g]]} if tampered and g in bad_groups else set()) for g, (kd, ix) in enumerate(zip(kinds, idxs))]
        rhos = [_rhos(rnd, len(r)) for r in recs]
        groups = [_group(kd, r, b"".join(w)) for kd, r, w in zip(kinds, recs, rhos)]
        got = gpu.r1cs_verify_mixed_combined(gens, groups)
        assert got == _weighted_sum([x for r in recs for x in r], [x for w in rhos for x in w]), tampered
        assert (got == IDENT) == (not tampered)
        opts(screen_batch=2560, stream_lanes=3)
        oks, nf = gpu.r1cs_verify_mixed_screened(gens, groups)
        assert oks == [[x["ok"] for x in r] for r in recs]
        assert nf == (2 if tampered else 0)
    recs[36] = [_off_curve(recs[36][0])] + recs[36][1:]
    groups[36] = _group(kinds[36], recs[36], b"".join(rhos[36]))
    assert gpu.r1cs_verify_mixed_combined(gens, groups) == POISON
    assert gpu.input_flag() == 1
    oks, nf = gpu.r1cs_verify_mixed_screened(gens, groups)
    assert oks == [[x["ok"] for x in r] for r in recs] and oks[36][0] == 0
    assert nf == 2                                 # (group 36 lies in check 2, which already falls back)
