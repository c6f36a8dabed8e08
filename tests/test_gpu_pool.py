"""bpgpu_pool_* -- queues of independent proofs over several slots (a context and a host thread each) from one process -- against the
oracle's accept bits and against the single-context entry points on a plain context.  The workload is the 8-bit range gadget with
8-bit window tables, in batches of 16 over three lanes; the lists [0], [0, 0] and [0, 0, 0] put one to three slots on ONE device (the
rehearsal a one-GPU machine allows), [0, 1] runs where there are two.  Run with `-m gpu` on an MI355X."""
import random
import threading

import pytest

import bp_helpers as bh
import circuit_gen as cg
import mpc_dealer as md
import oracle_lib as o
import prove_fs_cases as pc

pytestmark = pytest.mark.gpu
NB = 150
TAMPER = (0, 15, 16, 63, 64, 111, 112, 149)     # the ends of the shares of the 4 / 3 / 3-batch split: every slot holds bad and good proofs
LABEL = b"RangeProofTest"
OPTS = dict(stream_batch=16, stream_lanes=3, screen_batch=16)


@pytest.fixture(scope="module")
def m():
    import mpc_bulletproof_amd as mod
    return mod


class Work:
    """150 valid proofs and their tampered twins as per-proof operand triples, the oracle's verdicts, the circuit's shape"""

    def __init__(self):
        good, self.cap = bh.make_range_batch(8, NB)
        bad, _ = bh.make_range_batch(8, NB, tamper=set(range(NB)))
        self.good, self.bad, self.bad_rc = [], [], []
        for recs, out in ((good, self.good), (bad, self.bad)):
            for proof, com in recs:
                s = o.VerifySession(o.K_RANGE, 8, LABEL, [], com, proof, self.cap)
                _, p, q = bh.verify_inputs(proof, com)
                out.append((p, q, s.challenges()))
                if out is self.bad:
                    self.bad_rc.append(s.rc)
                s.close()
        s0 = o.VerifySession(o.K_RANGE, 8, LABEL, [], good[0][1], good[0][0], self.cap)
        self.csr, self.n, self.n1, self.k, self.m = s0.csr(), s0.n1 + s0.n2, s0.n1, s0.k, s0.m
        s0.close()
        self.nvar = 11 + self.m + 2 * self.k
        rnd = random.Random(4242)
        self.rho = b"".join(o.s2b(rnd.randrange(1, o.N)) for _ in range(NB))

    def queue(self, tamper=(), nb=NB):
        """-> (points, scalars, challenges, the oracle's accept bits)"""
        pick = [self.bad[i] if i in tamper else self.good[i] for i in range(nb)]
        want = [0 if (i in tamper and self.bad_rc[i] != 0) else 1 for i in range(nb)]
        return tuple(b"".join(x[j] for x in pick) for j in range(3)) + (want,)


@pytest.fixture(scope="module")
def work():
    return Work()


@pytest.fixture(scope="module")
def plain(m, work):
    """a plain context with the same tables, circuit and options: the single-context side of every comparison"""
    gpu = m.BpGpu(0)
    for k, v in OPTS.items():
        gpu.set_option(k, v)
    g = gpu.gens_create(o.gens("G", work.cap), o.gens("H", work.cap), o.generator(), o.generator(), 8)
    c = gpu.circuit_create(*work.csr, work.n, work.m)
    yield gpu, g, c
    gpu.gens_destroy(g)
    gpu.circuit_destroy(c)
    gpu.close()


def open_pool(m, work, devices):
    pool = m.BpPool(devices)
    for k, v in OPTS.items():
        pool.set_option(k, v)
    g = pool.gens_create(o.gens("G", work.cap), o.gens("H", work.cap), o.generator(), o.generator(), 8)
    c = pool.circuit_create(*work.csr, work.n, work.m)
    return pool, g, c


def close_pool(pool, g, c):
    pool.gens_destroy(g)
    pool.circuit_destroy(c)
    pool.close()


@pytest.fixture(scope="module")
def pools(m, work):
    """pools by device list, opened on first use and shared by the tests of this module"""
    made = {}

    def get(*devices):
        if devices not in made:
            made[devices] = open_pool(m, work, list(devices))
        return made[devices]
    yield get
    for p in made.values():
        close_pool(*p)


def sizes(lo):
    return [b - a for a, b in zip(lo, lo[1:])]


# ------------------------------------------------------------------------------------------------ stream verification
@pytest.mark.parametrize("devices", ((0,), (0, 0), (0, 0, 0)), ids=lambda d: "x".join(map(str, d)))
def test_stream_verdicts_equal_the_oracle_and_one_context(m, work, plain, pools, devices):
    pool, g, c = pools(*devices)
    gpu, g1, c1 = plain
    pts, sc, ch, want = work.queue(TAMPER)
    assert want == [0 if i in TAMPER else 1 for i in range(NB)]          # (the oracle rejects every tampered proof)
    for rep in range(2):                                                 # (the second call reuses the slots' lanes)
        ok, per = pool.r1cs_verify_stream(g, c, NB, work.n1, work.k, pts, sc, ch, want_shares=True)
        assert ok == want, rep
        assert per == sizes(m.lib.pool_shares(NB, len(devices), 16))
    ok1, _, _ = gpu.r1cs_verify_batch(g1, c1, NB, work.n1, work.k, work.m, pts, sc, ch, False, False)
    assert list(ok1) == want
    assert pool.r1cs_verify_stream(g, c, NB, work.n1, work.k, pts, sc, ch, raw=True) == b"".join(v.to_bytes(4, "little") for v in want)
    if len(devices) == 3:
        assert per == [64, 48, 38]
        # five proofs on three slots: one granule, two empty shares
        p5, s5, c5, w5 = work.queue({0, 4}, 5)
        ok, per = pool.r1cs_verify_stream(g, c, 5, work.n1, work.k, p5, s5, c5, want_shares=True)
        assert ok == w5 == [0, 1, 1, 1, 0] and per == [5, 0, 0]
    assert pool.r1cs_verify_stream(g, c, 0, work.n1, work.k, b"", b"", b"") == []


def test_stream_from_page_locked_operands(m, work, pools):
    """operands in bpgpu_host_alloc memory, allocated under device 0: both slots of [0, 0] own them and may read them in place (the
    second from an interior address); the verdicts do not depend on the route"""
    pool, g, c = pools(0, 0)
    pts, sc, ch, want = work.queue(TAMPER)
    bufs = [m.lib.host_alloc(len(b), b) for b in (pts, sc, ch)]
    try:
        assert pool.r1cs_verify_stream(g, c, NB, work.n1, work.k, *bufs) == want
    finally:
        for b in bufs:
            m.lib.host_free(b)


def test_a_malformed_proof_is_rejected_alone(m, work, pools):
    """an off-curve point in one proof of the MIDDLE slot's share: ok = 0 for that proof alone, and the call succeeds"""
    pool, g, c = pools(0, 0, 0)
    pts, sc, ch, _ = work.queue()
    victim = 80                                                          # share [64, 112)
    off = (victim * work.nvar + 1) * 64                                  # its second point: y := y + 1 leaves the curve
    y = (int.from_bytes(pts[off + 32:off + 64], "little") + 1) % (1 << 251)
    pts = pts[:off + 32] + y.to_bytes(32, "little") + pts[off + 64:]
    assert pool.r1cs_verify_stream(g, c, NB, work.n1, work.k, pts, sc, ch) == [0 if i == victim else 1 for i in range(NB)]


# ------------------------------------------------------------------------------------------------ screened verification
def test_screened(m, work, pools):
    pool, g, c = pools(0, 0, 0)
    pts, sc, ch, _ = work.queue()
    assert pool.r1cs_verify_screened(g, c, NB, work.n1, work.k, pts, sc, ch, work.rho) == ([1] * NB, 0)
    pts, sc, ch, want = work.queue({77})
    ok, nf = pool.r1cs_verify_screened(g, c, NB, work.n1, work.k, pts, sc, ch, work.rho)
    assert ok == want == pool.r1cs_verify_stream(g, c, NB, work.n1, work.k, pts, sc, ch) and nf == 1
    # an all-zero weight buffer accepts nothing: every check of every slot goes to the per-proof path
    ok, nf = pool.r1cs_verify_screened(g, c, NB, work.n1, work.k, pts, sc, ch, bytes(32 * NB))
    assert ok == want and nf == (NB + 15) // 16


# ------------------------------------------------------------------------------------------------ combined check
@pytest.mark.parametrize("devices", ((0, 0), (0, 0, 0)), ids=lambda d: "x".join(map(str, d)))
def test_combined_point_equals_one_context_over_the_whole_queue(m, work, plain, pools, devices):
    pool, g, c = pools(*devices)
    gpu, g1, c1 = plain
    pts, sc, ch, _ = work.queue()
    assert pool.r1cs_verify_combined(g, c, NB, work.n1, work.k, pts, sc, ch, work.rho) == bytes(64)
    pts, sc, ch, _ = work.queue({111})
    one = gpu.r1cs_verify_combined(g1, c1, NB, work.n1, work.k, work.m, pts, sc, ch, work.rho)
    assert one != bytes(64)
    assert pool.r1cs_verify_combined(g, c, NB, work.n1, work.k, pts, sc, ch, work.rho) == one


# ------------------------------------------------------------------------------------------------ prover
def test_provers_dealt_over_three_slots_equal_one_call(m, plain):
    """seven provers of a small one-phase generated circuit on [0, 0, 0] (shares 3 / 2 / 2): every output byte equals one
    bpgpu_r1cs_prove_fs on a plain context, and the wire proofs verify"""
    gpu, _, _ = plain
    nb, cap = 7, 8
    circ = cg.Circuit(4711, 3, 0, 2, 7, 0, "sparse")
    n, mm = circ.n, circ.m
    k = pc.lg_padded(n)
    plen = 1 + 11 * 32 + (2 * k + 2) * 32
    rnd = random.Random(99)
    rs = lambda cnt: b"".join(md.mont(rnd.randrange(cg.N)) for _ in range(cnt))      # noqa: E731
    wit = lambda v: b"".join(md.mont(x % cg.N) for x in v) * nb                       # noqa: E731
    init = bytes(rnd.getrandbits(8) for _ in range(32 * nb))
    v, vb = wit(circ.v), rs(nb * mm)
    gens = (o.gens("G", cap), o.gens("H", cap), o.generator(), o.generator(), 8)
    g1, c1 = gpu.gens_create(*gens), gpu.circuit_create(*circ.csr(), n, mm)
    pool = m.BpPool([0, 0, 0])
    pg, pcirc = pool.gens_create(*gens), pool.circuit_create(*circ.csr(), n, mm)
    try:
        _, Vc, states = gpu.r1cs_commit_values(g1, nb, mm, v, vb, init, want_points=False)
        kw = dict(states=states, a_L=wit(circ.a_L[:n]), a_R=wit(circ.a_R[:n]), a_O=wit([circ.a_L[i] * circ.a_R[i] for i in range(n)]),
                  blindings=rs(8 * nb), v_blinding=vb)
        for src in (dict(s_L=rs(nb * n), s_R=rs(nb * n)), dict(vector_keys=bytes(rnd.getrandbits(8) for _ in range(32 * nb)))):
            one = gpu.r1cs_prove_fs(g1, c1, nb, n, mm, **kw, **src)
            got = pool.r1cs_prove_fs(pg, pcirc, nb, n, mm, **kw, **src)
            for name, a, b in zip(("points", "scalars", "wire", "challenges", "states"), got, one):
                assert a == b, name
            assert gpu.r1cs_verify_batch_wire(g1, c1, nb, n, plen, got[2], Vc, init) == [1] * nb
        assert m.lib.pool_shares(nb, 3, 1) == [0, 3, 5, 7]
        # the refusals come before any worker is woken, with the single-context codes
        with pytest.raises(m.BpGpuError) as e:
            pool.r1cs_prove_fs(pg, pcirc, nb, n, mm, **kw)                            # no source of s_L, s_R
        assert e.value.code == m.lib.E_ARG and "refused before any slot was woken" in str(e.value)
    finally:
        pool.gens_destroy(pg)
        pool.circuit_destroy(pcirc)
        pool.close()
        gpu.gens_destroy(g1)
        gpu.circuit_destroy(c1)


# ------------------------------------------------------------------------------------------------ handles
def test_handles_borrowed_contexts_and_options(m, work, pools):
    pool, g, c = pools(0, 0)
    assert pool.slots() == 2 and [pool.device(s) for s in range(2)] == [0, 0] and pool.device(2) == m.lib.E_ARG
    assert pool.gens_get(g, 0) and pool.gens_get(g, 0) == pool.gens_get(g, 1) and pool.gens_get(g, 2) is None
    assert pool.circuit_get(c, 0) and pool.circuit_get(c, 0) == pool.circuit_get(c, 1) and pool.circuit_get(c, 2) is None
    pts, sc, ch, want = work.queue(TAMPER)
    assert pool.r1cs_verify_stream(g, c, NB, work.n1, work.k, pts, sc, ch) == want
    # a borrowed context serves a plain single-context call with the slot's handles
    ctx1 = pool.ctx(1)
    assert [ctx1.get_option(k) for k in OPTS] == list(OPTS.values())
    ok, _, _ = ctx1.r1cs_verify_batch(pool.gens_get(g, 1), pool.circuit_get(c, 1), NB, work.n1, work.k, work.m, pts, sc, ch, False, False)
    assert list(ok) == want
    ctx1.close()                                                         # (borrowed: the context stays the pool's)
    assert pool.r1cs_verify_stream(g, c, NB, work.n1, work.k, pts, sc, ch) == want
    with pytest.raises(m.BpGpuError):
        pool.ctx(2)
    # an option value that a slot refuses leaves every slot as it was
    with pytest.raises(m.BpGpuError) as e:
        pool.set_option("stream_lanes", 0)
    assert e.value.code == m.lib.E_ARG
    assert [pool.ctx(s).get_option("stream_lanes") for s in range(2)] == [3, 3]
    # shape errors: the single-context codes, before any worker is woken
    for kw, code in ((dict(k=32), m.lib.E_LEN), (dict(n1=work.n + 1), m.lib.E_LEN), (dict(k=work.k + 1), m.lib.E_LEN)):
        a = dict(n1=work.n1, k=work.k)
        a.update(kw)
        with pytest.raises(m.BpGpuError) as e:
            pool.r1cs_verify_stream(g, c, NB, a["n1"], a["k"], pts, sc, ch)
        assert e.value.code == code and "bpgpu_pool_r1cs_verify_stream" in str(e.value), kw
    other, g2, c2 = pools(0)
    with pytest.raises(m.BpGpuError) as e:                               # handles of another pool
        pool.r1cs_verify_stream(g2, c2, NB, work.n1, work.k, pts, sc, ch)
    assert e.value.code == m.lib.E_ARG


def test_destroy_then_create_again(m, work):
    pts, sc, ch, want = work.queue({1}, 5)
    for rep in range(2):
        pool, g, c = open_pool(m, work, [0, 0])
        try:
            assert pool.r1cs_verify_stream(g, c, 5, work.n1, work.k, pts, sc, ch) == want, rep
        finally:
            close_pool(pool, g, c)


def test_two_threads_on_one_pool(m, work, pools):
    """a pool serialises its calls: two Python threads on one pool both get their own, correct verdicts"""
    pool, g, c = pools(0, 0)
    queues = [work.queue(TAMPER), work.queue({5, 100})]
    got = [None, None]

    def run(i):
        pts, sc, ch, _ = queues[i]
        got[i] = [pool.r1cs_verify_stream(g, c, NB, work.n1, work.k, pts, sc, ch) for _ in range(3)]
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for i in range(2):
        assert got[i] == [queues[i][3]] * 3, i


# ------------------------------------------------------------------------------------------------ two devices
def test_two_devices(m, work, plain):
    if m.lib.device_count() < 2:
        pytest.skip("needs two GPUs: this machine has %d (the lists [0, 0] and [0, 0, 0] above rehearse the pool on one)" % m.lib.device_count())
    gpu, g1, c1 = plain
    pool, g, c = open_pool(m, work, [0, 1])
    try:
        assert [pool.device(s) for s in range(2)] == [0, 1] and pool.gens_get(g, 0) != pool.gens_get(g, 1)
        pts, sc, ch, want = work.queue(TAMPER)                           # pageable operands
        ok, per = pool.r1cs_verify_stream(g, c, NB, work.n1, work.k, pts, sc, ch, want_shares=True)
        assert ok == want and per == [80, 70]
        assert pool.r1cs_verify_combined(g, c, NB, work.n1, work.k, *work.queue()[:3], work.rho) == bytes(64)
        pts, sc, ch, _ = work.queue({111})
        one = gpu.r1cs_verify_combined(g1, c1, NB, work.n1, work.k, work.m, pts, sc, ch, work.rho)
        assert pool.r1cs_verify_combined(g, c, NB, work.n1, work.k, pts, sc, ch, work.rho) == one != bytes(64)
    finally:
        close_pool(pool, g, c)
