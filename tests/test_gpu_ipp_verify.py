"""GPU tests of the batched InnerProductProof::verify (bpgpu_ipp_verify_batch / _batch_dev / _gens / _fs): accept bits and expect_P
against the CPU oracle, bit for bit.  Run with `-m gpu` on an MI355X.

The proofs come from the oracle (ipp_verify_cases.make, spread over spawned worker processes: they never see the GPU); the
oracle's own ipp_verify gives the expected bit of every proof, tampered ones included."""
import concurrent.futures
import multiprocessing
import os

import pytest

import ipp_verify_cases as cases
import oracle_lib as o

pytestmark = pytest.mark.gpu
H = bytes.fromhex
N = o.N


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def maker():
    """make(list of (n, seed, rot, tamper)) -> the proofs, cached by their arguments, the new ones made in parallel"""
    cache = {}
    workers = max(1, min(16, os.cpu_count() or 1))
    pool = concurrent.futures.ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context("spawn"))

    def make(keys):
        new = [k for k in dict.fromkeys(keys) if k not in cache]
        if len(new) > 2 and new[0][0] >= 64:
            cache.update(zip(new, pool.map(cases.make, new)))
        else:
            cache.update((k, cases.make(k)) for k in new)
        return [cache[k] for k in keys]
    yield make
    pool.shutdown()


def J(c, k):
    return b"".join(map(H, c[k]))


def cat(recs, key):
    return b"".join(r[key] for r in recs)


def batch_args(recs, shared):
    """positional operands of BpGpu.ipp_verify_batch after (nb, n)"""
    return (cat(recs, "Q"), cat(recs, "Gf"), cat(recs, "Hf"), recs[0]["G"] if shared else cat(recs, "G"),
            recs[0]["H"] if shared else cat(recs, "H"), shared, cat(recs, "P"), cat(recs, "L"), cat(recs, "R"), cat(recs, "ab"), cat(recs, "ch"))


def tamper_plan(nb, n, case_index):
    """{proof index: kind}: a fixed subset of at most half the batch.  70 proofs carry every kind once; 7 proofs have room for three,
    which rotate through the kinds with the case, so that the nb = 7 cases together cover all of them too.  A proof of length 1 has
    no L, R or challenge to change."""
    kinds = [k for k in cases.KINDS if n > 1 or k in ("a", "b", "P", "Gf")]
    if nb >= 2 * len(cases.KINDS):
        return {3 + 7 * i: k for i, k in enumerate(kinds)}
    slots = nb // 2
    return {1 + 2 * i: kinds[(3 * case_index + i) % len(kinds)] for i in range(slots)}


# ------------------------------------------------------------------ 1. golden
def test_golden_create_cases_accept_and_swaps_reject(gpu, golden_ipp):
    for c in golden_ipp["create"]:
        n = c["n"]
        Gp, Hp = o.gens("G", n), o.gens("H", n)
        L, R, a, b, ch = J(c, "L"), J(c, "R"), H(c["a_out"]), H(c["b_out"]), J(c, "challenges")
        oargs = (H(c["label"]), n, J(c, "G_factors"), J(c, "H_factors"), H(c["P"]), H(c["Q"]), Gp, Hp)

        def gpu_bit(L, R, a, b, ch):
            return gpu.ipp_verify_batch(1, n, H(c["Q"]), J(c, "G_factors"), J(c, "H_factors"), Gp, Hp, True, H(c["P"]), L, R, a + b, ch)[0]
        assert gpu_bit(L, R, a, b, ch) == 1 and o.ipp_verify(*oargs, L, R, a, b) == 0
        if n > 1:
            assert gpu_bit(L, R, b, a, ch) == (1 if o.ipp_verify(*oargs, L, R, b, a) == 0 else 0) == 0
            # L and R swapped: the host's replay of the proof as received gives other challenges; with the original ones it is wrong too
            assert o.ipp_verify(*oargs, R, L, a, b) == -1
            assert gpu_bit(R, L, a, b, cases.replay(n, R, L)[0] if H(c["label"]) == cases.LABEL else ch) == 0
            assert gpu_bit(R, L, a, b, ch) == 0


# ------------------------------------------------------------------ 2. batched
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("n", [1, 2, 8, 64, 1024])
@pytest.mark.parametrize("nb", [1, 7, 70])
def test_batches_with_tampered_proofs(gpu, maker, nb, n, shared):
    case_index = [1, 2, 8, 64, 1024].index(n)
    plan = tamper_plan(nb, n, case_index)
    assert len(plan) <= nb // 2
    recs = maker([(n, 100 * case_index + p, 0 if shared else p, plan.get(p)) for p in range(nb)])
    want = [r["bit"] for r in recs]
    if nb >= 7:
        assert 0 in want and 1 in want          # the oracle alone produces both outcomes
    assert want == [0 if p in plan else 1 for p in range(nb)]
    ok, expect = gpu.ipp_verify_batch(nb, n, *batch_args(recs, shared), want_expect=True)
    assert ok == want
    for p, r in enumerate(recs):
        assert expect[64 * p:64 * p + 64] == r["expect"], p
    assert gpu.ipp_verify_batch(nb, n, *batch_args(recs, shared)) == want      # without expect_P


# ------------------------------------------------------------------ 3. bucket-method sizes
def _gpu_create(gpu, nb, n, Q, Gf, Hf, G, Hh, shared, a, b):
    """InnerProductProof::create on the GPU with the transcript on the device -> per proof L, R, a, b"""
    import pymodel as pm
    k = n.bit_length() - 1
    t = pm.Transcript(cases.LABEL)
    t.innerproduct_domain_sep(n)
    s = gpu.ipp_begin(nb, n, Q, Gf, Hf, G, Hh, shared, a, b)
    try:
        L, R, aa, bb, _ = gpu.ipp_run_fs(s, nb, k, t.state * nb)
    finally:
        gpu.ipp_destroy(s)
    return L, R, aa, bb


@pytest.mark.parametrize("nb,n,shared,tampered", [(1, 1 << 16, True, None), (3, 1 << 12, False, 1)])
def test_bucket_method_sizes(gpu, nb, n, shared, tampered):
    """Proofs of 2^16 and 3 x 2^12 multipliers, created on the GPU (the oracle needs minutes for one of them); the verdicts are
    checked against the oracle's ipp_verify, which replays its own transcript."""
    k = n.bit_length() - 1
    # generator sets tiled from chains of 4096 (the oracle derives 2^16 generators in half a minute), per-proof sets rotated
    base = cases.gens(4096)

    def tiled(chain, rot):
        t = chain * (n // 4096)
        return t[64 * rot:] + t[:64 * rot]
    G, Hh = zip(*((tiled(base[0], 5 * p), tiled(base[1], 5 * p + 7)) for p in range(nb)))
    a, b, Gf, Hf = (o.random_scalars(7000 + j, nb * n) for j in range(4))
    Q = b"".join(o.point_mul(o.random_scalars(7100 + p, 1), o.generator()) for p in range(nb))
    Gall, Hall = (G[0], Hh[0]) if shared else (b"".join(G), b"".join(Hh))
    L, R, aa, bb = _gpu_create(gpu, nb, n, Q, Gf, Hf, Gall, Hall, shared, a, b)
    P = b""
    for p in range(nb):
        sl = slice(32 * n * p, 32 * n * (p + 1))
        P += o.msm(o.sc_binop(2, a[sl], Gf[sl]) + o.sc_binop(2, b[sl], Hf[sl]) + o.inner_product(a[sl], b[sl]),
                   G[p] + Hh[p] + Q[64 * p:64 * p + 64])
    if tampered is not None:
        aa = aa[:32 * tampered] + o.sc_binop(0, aa[32 * tampered:32 * tampered + 32], o.s2b(1)) + aa[32 * tampered + 32:]
    want, ch, ab = [], b"", b""
    for p in range(nb):
        sl = slice(32 * n * p, 32 * n * (p + 1))
        Lp, Rp = L[64 * k * p:64 * k * (p + 1)], R[64 * k * p:64 * k * (p + 1)]
        want.append(1 if o.ipp_verify(cases.LABEL, n, Gf[sl], Hf[sl], P[64 * p:64 * p + 64], Q[64 * p:64 * p + 64], G[p], Hh[p], Lp, Rp,
                                      aa[32 * p:32 * p + 32], bb[32 * p:32 * p + 32]) == 0 else 0)
        ch += cases.replay(n, Lp, Rp)[0]
        ab += aa[32 * p:32 * p + 32] + bb[32 * p:32 * p + 32]
    assert want == [0 if p == tampered else 1 for p in range(nb)]
    assert gpu.ipp_verify_batch(nb, n, Q, Gf, Hf, Gall, Hall, shared, P, L, R, ab, ch) == want


# ------------------------------------------------------------------ 4. resident generators
@pytest.mark.parametrize("n,cap,c", [(8, 16, 4), (64, 128, 8), (1024, 2048, 4)])
def test_resident_generators(gpu, maker, n, cap, c):
    nb = 5
    plan = {1: "a", 3: "R"}
    recs = maker([(n, 900 + p, 0, plan.get(p)) for p in range(nb)])
    want = [r["bit"] for r in recs]
    assert want == [1, 0, 1, 0, 1]
    B = o.generator()
    g = gpu.gens_create(o.gens("G", cap), o.gens("H", cap), B, B, c)
    try:
        ok, expect = gpu.ipp_verify_gens(g, nb, n, cat(recs, "w"), cat(recs, "Gf"), cat(recs, "Hf"), cat(recs, "P"), cat(recs, "L"),
                                         cat(recs, "R"), cat(recs, "ab"), cat(recs, "ch"), want_expect=True)
    finally:
        gpu.gens_destroy(g)
    ok2, expect2 = gpu.ipp_verify_batch(nb, n, *batch_args(recs, True), want_expect=True)
    assert ok == ok2 == want
    assert expect == expect2 == cat(recs, "expect")


def test_resident_generators_capacity(gpu):
    import mpc_bulletproof_amd as m
    B = o.generator()
    g = gpu.gens_create(o.gens("G", 4), o.gens("H", 4), B, B, 8)
    try:
        z = bytes(64 * 8 * 3)
        with pytest.raises(m.BpGpuError) as e:
            gpu.ipp_verify_gens(g, 1, 8, z[:32], z[:256], z[:256], z[:64], z[:192], z[:192], z[:64], z[:96])
        assert e.value.code == m.lib.E_GENS
    finally:
        gpu.gens_destroy(g)


# ------------------------------------------------------------------ 5. device transcript
@pytest.mark.parametrize("resident", [True, False])
def test_device_transcript(gpu, maker, resident):
    import pymodel as pm
    nb, n = 6, 32
    plan = {2: "b", 4: "L"}
    recs = maker([(n, 1200 + p, 0, plan.get(p)) for p in range(nb)])
    recs = [dict(r) for r in recs]
    k = n.bit_length() - 1
    recs[5]["L"] = recs[5]["L"][:64 * 2] + bytes(64) + recs[5]["L"][64 * 3:]      # an identity L: rejected by validate_and_append_point
    want = [r["bit"] for r in recs]
    want[5] = 1 if o.ipp_verify(cases.LABEL, n, recs[5]["Gf"], recs[5]["Hf"], recs[5]["P"], recs[5]["Q"], recs[5]["G"], recs[5]["H"],
                                recs[5]["L"], recs[5]["R"], recs[5]["ab"][:32], recs[5]["ab"][32:]) == 0 else 0
    assert want == [1, 1, 0, 1, 0, 0]
    t = pm.Transcript(cases.LABEL)
    t.innerproduct_domain_sep(n)
    B = o.generator()
    g = gpu.gens_create(o.gens("G", n), o.gens("H", n), B, B, 8) if resident else None
    try:
        ok, states = gpu.ipp_verify_fs(g, nb, n, cat(recs, "w" if resident else "Q"), cat(recs, "Gf"), cat(recs, "Hf"),
                                       None if resident else recs[0]["G"], None if resident else recs[0]["H"], True, cat(recs, "P"),
                                       cat(recs, "L"), cat(recs, "R"), cat(recs, "ab"), t.state * nb)
    finally:
        if g is not None:
            gpu.gens_destroy(g)
    assert ok == want
    for p in range(nb - 1):          # (the chain of the proof with the identity point ends where the oracle's replay fails)
        assert states[32 * p:32 * p + 32] == recs[p]["state"], p


# ------------------------------------------------------------------ 6. device pointers
def test_dev_form_and_malformed_operands(gpu, maker):
    import mpc_bulletproof_amd as m
    nb, n, k = 4, 16, 4
    recs = maker([(n, 1300 + p, 0, {2: "P"}.get(p)) for p in range(nb)])
    args = batch_args(recs, True)
    want, expect = gpu.ipp_verify_batch(nb, n, *args, want_expect=True)
    assert want == [1, 1, 0, 1]

    def run_dev(args):
        ptrs = [gpu.to_device(x) if isinstance(x, bytes) else x for x in args]
        d_ok, d_ex = gpu.malloc(4 * nb), gpu.malloc(64 * nb)
        try:
            gpu.ipp_verify_batch_dev(nb, n, k, *ptrs, d_ok, d_ex)
            gpu.sync()
            flag = gpu.input_flag()
            return flag, [int.from_bytes(gpu.download(d_ok, 4 * nb)[4 * i:4 * i + 4], "little") for i in range(nb)], gpu.download(d_ex, 64 * nb)
        finally:
            for p in ptrs + [d_ok, d_ex]:
                if not isinstance(p, bool):
                    gpu.free(p)
    assert run_dev(args) == (0, want, expect)
    # a non-canonical scalar (b of proof 1 := the group order) and an off-curve point (R_0 of proof 3: y + 1)
    ab = args[9]
    bad_scalar = args[:9] + (ab[:96] + N.to_bytes(32, "little") + ab[128:],) + args[10:]
    R = bytearray(args[8])
    R[64 * k * 3 + 32] ^= 1
    bad_point = args[:8] + (bytes(R),) + args[9:]
    for bad in (bad_scalar, bad_point):
        assert run_dev(bad)[0] != 0
        with pytest.raises(m.BpGpuError) as e:
            gpu.ipp_verify_batch(nb, n, *bad)
        assert e.value.code == m.lib.E_ARG
    assert run_dev(args) == (0, want, expect)          # the flag reports on the most recent call


# ------------------------------------------------------------------ 7. zero challenge
def test_zero_challenge_rejects_without_an_error(gpu, maker):
    nb, n = 3, 8
    recs = [dict(r) for r in maker([(n, 1400 + p, 0, None) for p in range(nb)])]
    recs[1]["ch"] = recs[1]["ch"][:32] + bytes(32) + recs[1]["ch"][64:]
    assert gpu.ipp_verify_batch(nb, n, *batch_args(recs, True)) == [1, 0, 1]
