"""Generated circuits (tests/circuit_gen.py) on every GPU path that takes a caller's CSR constraint system, against the Python model
(oracle/pymodel.py) on integers: constraint flattening, the refusals of circuit_create*, the prover's polynomials, the verifier's
scalar assembly in each of its kernels, whole proofs, and circuits without multipliers or rows.  Run with `-m gpu` on an MI355X."""
import random

import pytest

import circuit_gen as cg
import mpc_dealer as md
import oracle_lib as o
from polys_model import model_polys, padded

pm = cg.pm
N = pm.N
pytestmark = pytest.mark.gpu
CAP = 128
IDENT = bytes(64)
le = md.le


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


class ModelGens:
    """the model's BulletproofGens interface over the oracle's generator chain (the model builds each generator with a Python scalar
    multiplication; the first ones are checked to be the same points)"""

    def __init__(self, cap):
        self.gens_capacity = cap
        self.gb, self.hb = o.gens("G", cap), o.gens("H", cap)
        self._g = [pm.b2p(b) for b in md.cut(self.gb, 64)]
        self._h = [pm.b2p(b) for b in md.cut(self.hb, 64)]
        ref = pm.BulletproofGens(2)
        assert self._g[:2] == ref.G(2) and self._h[:2] == ref.H(2) and o.generator() == pm.p2b(pm.G)

    def G(self, n, share=0):
        return self._g[:n]

    def H(self, n, share=0):
        return self._h[:n]


@pytest.fixture(scope="module")
def mgens():
    return ModelGens(CAP)


def ints(b):
    return [int.from_bytes(x, "little") for x in md.cut(b, 32)]


def pack(vals):
    return b"".join(le(v) for v in vals)


def make(gpu, circ, ark=False):
    if circ.nchi:
        return gpu.circuit_create_param(circ.q, circ.nchi, *circ.csr_param(), circ.n, circ.m)
    return gpu.circuit_create(*circ.csr(ark), circ.n, circ.m, ark=ark)


# ------------------------------------------------------------------------------------------------ flattening
def check_flatten(gpu, circ, h, zs):
    n, m = circ.n, circ.m
    got = gpu.flatten_constraints(h, n, m, pack(zs))
    for p, z in enumerate(zs):
        wL, wR, wO, wV, wc = cg.model_weights(circ, z)
        assert ints(got[0])[p * n:(p + 1) * n] == wL, ("wL", p, hex(z))
        assert ints(got[1])[p * n:(p + 1) * n] == wR, ("wR", p, hex(z))
        assert ints(got[2])[p * n:(p + 1) * n] == wO, ("wO", p, hex(z))
        assert ints(got[3])[p * m:(p + 1) * m] == wV, ("wV", p, hex(z))
        assert ints(got[4])[p] == wc, ("wc", p, hex(z))


# every n of {1, 2, 3, 5, 13, 33, 63, 64, 65, 100}, m of {0, 1, 5, 64, 65, 70}, q of {1, 7, 40, 257, 300} and every profile occurs
FLATTEN_SHAPES = [
    ("sparse", 1, 0, 1), ("sparse", 2, 1, 7), ("sparse", 3, 5, 40), ("sparse", 65, 64, 257), ("sparse", 100, 70, 300),
    ("dense", 1, 1, 1), ("dense", 5, 0, 7), ("dense", 13, 5, 40), ("dense", 33, 1, 257), ("dense", 63, 65, 40), ("dense", 64, 64, 7),
    ("dense", 100, 70, 300),
    ("columns", 13, 65, 300), ("columns", 33, 5, 257), ("columns", 64, 70, 300), ("columns", 100, 64, 40), ("columns", 65, 1, 300),
    ("columns+edge_coeff", 64, 64, 300), ("columns+edge_coeff", 13, 5, 257), ("dense+edge_coeff", 5, 5, 40), ("dense+edge_coeff", 63, 0, 7),
    ("sparse+edge_coeff", 2, 1, 300),
    ("dups", 3, 1, 7), ("dups", 33, 5, 40), ("dense+dups", 13, 5, 257),
    ("holes", 2, 0, 1), ("holes", 5, 5, 7), ("holes", 64, 65, 257), ("holes", 100, 1, 300),
    ("columns+holes+edge_coeff+dups", 65, 70, 300),
]


@pytest.mark.parametrize("profile,n,m,q", FLATTEN_SHAPES)
def test_flatten_generated_circuits(gpu, profile, n, m, q):
    """bpgpu_flatten_constraints on circuits from circuit_create and circuit_create_ark, one and three proofs a call, z in {1, 2, n - 1,
    random}, against pm.Verifier.flattened_constraints"""
    rnd = random.Random(n * 1000 + q)
    circ = cg.Circuit(n + 7 * m + q, n, 0, m, q, 0, profile)
    for ark in (False, True):
        h = make(gpu, circ, ark)
        try:
            for z in (1, 2, N - 1, rnd.randrange(N)):
                check_flatten(gpu, circ, h, [z])
            check_flatten(gpu, circ, h, [1, N - 1, rnd.randrange(N)])
            check_flatten(gpu, circ, h, [2, rnd.randrange(N), rnd.randrange(N)])
        finally:
            gpu.circuit_destroy(h)


def test_flatten_a_circuit_wider_than_one_scan_pass(gpu):
    """3 n + m + 2 = 4505 column pointers: every lane of the column scan owns a run of eight, two vector loads; sparse rows plus the
    columns of exact lengths, the 257-term one among them"""
    circ = cg.Circuit(4505, 1500, 0, 3, 700, 0, "sparse+columns")
    assert 3 * circ.n + circ.m + 2 > 4096 and 257 in circ.column_lengths.values()
    rnd = random.Random(4505)
    for ark in (False, True):
        h = make(gpu, circ, ark)
        try:
            check_flatten(gpu, circ, h, [rnd.randrange(N)])
            check_flatten(gpu, circ, h, [N - 1, 2, rnd.randrange(N)])
        finally:
            gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ refusals
def test_malformed_circuits_are_refused_and_the_context_stays_usable(gpu):
    import mpc_bulletproof_amd as m
    good = cg.Circuit(5, 4, 0, 3, 9, 0, "dense")
    rp, kd, ix, cf = good.csr()
    n, mm = good.n, good.m
    t_l = kd.index(0)
    t_v = kd.index(3)

    def with_(lst, t, v):
        return lst[:t] + [v] + lst[t + 1:]

    bad_rp = list(rp)
    bad_rp[2], bad_rp[3] = rp[3], rp[2]
    assert bad_rp[3] < bad_rp[2]
    par = cg.Circuit(6, 2, 1, 1, 4, 1, "sparse")
    prp, pkd, pix, pcf = par.csr_param()
    rows9 = prp + [prp[-1]] * (8 * par.q)                       # the row pointers of nine challenge blocks, eight of them empty
    cases = [
        ("kind 5", lambda: gpu.circuit_create(rp, with_(kd, t_l, 5), ix, cf, n, mm)),
        ("multiplier index n", lambda: gpu.circuit_create(rp, kd, with_(ix, t_l, n), cf, n, mm)),
        ("committed index m", lambda: gpu.circuit_create(rp, kd, with_(ix, t_v, mm), cf, n, mm)),
        ("coefficient n", lambda: gpu.circuit_create(rp, kd, ix, cf[:32 * t_l] + N.to_bytes(32, "little") + cf[32 * t_l + 32:], n, mm)),
        ("coefficient n, ark", lambda: gpu.circuit_create(rp, kd, ix, cf[:32 * t_l] + N.to_bytes(32, "little") + cf[32 * t_l + 32:], n, mm, ark=True)),
        ("row_ptr not monotone", lambda: gpu.circuit_create(bad_rp, kd, ix, cf, n, mm)),
        ("nchi 9", lambda: gpu.circuit_create_param(par.q, 9, rows9, pkd, pix, pcf, par.n, par.m)),
        ("kind 5, param", lambda: gpu.circuit_create_param(par.q, 1, prp, with_(pkd, 0, 5), pix, pcf, par.n, par.m)),
    ]
    rnd = random.Random(9)
    for name, call in cases:
        with pytest.raises(m.lib.BpGpuError) as e:
            call()
        assert e.value.code in (m.lib.E_ARG, m.lib.E_LEN), name
        h = make(gpu, good)
        try:
            check_flatten(gpu, good, h, [rnd.randrange(N), 1])
        finally:
            gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ prover polynomials
def random_witness(rnd, n):
    return {k: [rnd.randrange(N) for _ in range(n)] for k in ("aL", "aR", "aO", "sL", "sR")}


@pytest.mark.parametrize("profile,n,m,q", [("dense", 13, 5, 40), ("columns+edge_coeff", 33, 11, 300), ("dups", 5, 1, 7),
                                           ("dense+dups+holes", 3, 2, 5)])
def test_prover_polys_and_eval_on_generated_circuits(gpu, profile, n, m, q):
    """bpgpu_r1cs_prover_polys / _ark / _eval with the weights of the Python model: t_1..t_6, wV, l_vec and r_vec with their padding; y in
    {1, n - 1, random}"""
    rnd = random.Random(n + q)
    circ = cg.Circuit(31 + n, n, 0, m, q, 0, profile)
    h = make(gpu, circ)
    nb, np_ = 3, padded(n)
    try:
        ys, zs, xs = [1, N - 1, rnd.randrange(1, N)], [rnd.randrange(N) for _ in range(nb)], [rnd.randrange(N) for _ in range(nb)]
        wit = [random_witness(rnd, n) for _ in range(nb)]
        col = lambda k, f: b"".join(f(v) for w in wit for v in w[k])       # noqa: E731
        outs = []
        for f, ark in ((le, False), (md.mont, True)):
            sc = lambda vals: b"".join(f(v) for v in vals)       # noqa: E731
            t, wv, ses = gpu.r1cs_prover_polys(h, nb, n, m, sc(ys), sc([pow(y, -1, N) for y in ys]), sc(zs), col("aL", f), col("aR", f),
                                               col("aO", f), col("sL", f), col("sR", f), ark=ark)
            lv, rv = gpu.r1cs_prover_eval(ses, nb, np_, pack(xs))
            gpu.prover_destroy(ses)
            outs.append((t, wv, lv, rv))
        assert outs[0] == outs[1]
        t, wv, lv, rv = outs[0]
        for p in range(nb):
            weights = cg.model_weights(circ, zs[p])
            want_t, want_l, want_r = model_polys(circ, weights, ys[p], xs[p], wit[p])
            assert ints(t)[6 * p:6 * p + 6] == want_t, p
            assert ints(wv)[m * p:m * p + m] == weights[3], p
            assert ints(lv)[np_ * p:np_ * (p + 1)] == want_l, p
            assert ints(rv)[np_ * p:np_ * (p + 1)] == want_r, p
    finally:
        gpu.circuit_destroy(h)


@pytest.mark.parametrize("nchi,profile", [(1, "dense"), (2, "sparse+dups"), (3, "dense+edge_coeff"), (8, "dense+dups")])
def test_session_polys_param_on_generated_circuits(gpu, gens, nchi, profile):
    """the resident session (bpgpu_r1cs_prover_commit, then bpgpu_r1cs_prover_session_polys_param) on circuits affine in 1, 2, 3 and 8
    gadget challenges; one proof with every challenge 0, one with every challenge n - 1, one random"""
    rnd = random.Random(nchi)
    n1, n2, m, q = 4, 3, 2, 11
    circ = cg.Circuit(50 + nchi, n1, n2, m, q, nchi, profile)
    n, nb, np_ = n1 + n2, 3, 8
    h = make(gpu, circ)
    try:
        ys, zs, xs = [1, N - 1, rnd.randrange(1, N)], [rnd.randrange(N) for _ in range(nb)], [rnd.randrange(N) for _ in range(nb)]
        chis = [[0] * nchi, [N - 1] * nchi, [rnd.randrange(N) for _ in range(nchi)]]
        wit = [random_witness(rnd, n) for _ in range(nb)]
        col = lambda k: b"".join(md.mont(v) for w in wit for v in w[k])       # noqa: E731
        ses, _ = gpu.r1cs_prover_commit(gens, None, nb, n, col("aL"), col("aR"), col("aO"), b"".join(md.mont(rnd.randrange(N)) for _ in range(3 * nb)),
                                        col("sL"), col("sR"))
        try:
            t, wv = gpu.r1cs_prover_session_polys_param(ses, h, nb, m, pack(ys), pack(zs), pack([c for ch in chis for c in ch]))
            lv, rv = gpu.r1cs_prover_eval(ses, nb, np_, pack(xs))
        finally:
            gpu.prover_destroy(ses)
        for p in range(nb):
            weights = cg.model_weights(circ, zs[p], chis[p])
            want_t, want_l, want_r = model_polys(circ, weights, ys[p], xs[p], wit[p])
            assert ints(t)[6 * p:6 * p + 6] == want_t, p
            assert ints(wv)[m * p:m * p + m] == weights[3], p
            assert ints(lv)[np_ * p:np_ * (p + 1)] == want_l, p
            assert ints(rv)[np_ * p:np_ * (p + 1)] == want_r, p
    finally:
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ verifier scalars
_POOL = []


def some_points(rnd, count):
    """valid points: small multiples of the generator"""
    if not _POOL:
        acc = pm.G
        for _ in range(48):
            _POOL.append(acc)
            acc = pm.pt_add(acc, pm.G)
    return [rnd.choice(_POOL) for _ in range(count)]


def operands(proof, V, trace):
    """the operands of bpgpu_r1cs_verify_batch for one proof of the model and the challenges its transcript produced"""
    names = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2")
    pts = [proof[k] for k in names] + list(V) + [proof[k] for k in ("T_1", "T_3", "T_4", "T_5", "T_6")] + proof["L_vec"] + proof["R_vec"]
    sc = [proof[k] for k in ("t_x", "t_x_blinding", "e_blinding", "a", "b")]
    ch = [trace[k] for k in ("y", "z", "u", "x", "w", "r")] + trace["ipp_u"]
    return b"".join(pm.p2b(x) for x in pts), pack(sc), pack(ch)


def model_run(circ, mgens, proof, V, chi=None):
    """pm.Verifier.verification_msm -> (scalar bytes, mega_check bytes by the oracle's MSM over these scalars, operands, gadget challenges)"""
    vf, info = cg.verifier(circ, V, chi=chi)
    trace = {}
    scalars, points = vf.verification_msm(proof, mgens, trace)
    keep = [(s, pt) for s, pt in zip(scalars, points) if pt is not pm.INF]
    mega = o.msm(pack([s for s, _ in keep]), b"".join(pm.p2b(pt) for _, pt in keep))
    return pack(scalars), mega, operands(proof, V, trace), info["chi"]


def random_proof(rnd, circ):
    """not a valid proof: canonical random scalars and valid points in the places of a proof of this circuit's shape"""
    k = (padded(circ.n) - 1).bit_length()
    pts = some_points(rnd, 11 + 2 * k)
    proof = dict(zip(("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6"), pts))
    if not circ.two_phase:
        proof["A_I2"] = proof["A_O2"] = proof["S2"] = pm.INF
    proof["L_vec"], proof["R_vec"] = pts[11:11 + k], pts[11 + k:]
    for name in ("t_x", "t_x_blinding", "e_blinding", "a", "b"):
        proof[name] = rnd.randrange(N)
    return proof, some_points(rnd, circ.m)


def gpu_verify(gpu, gens, circ, h, recs, want_scalars=True):
    nb = len(recs)
    k = (padded(circ.n) - 1).bit_length()
    pts, sc, ch = (b"".join(r["ops"][i] for r in recs) for i in range(3))
    if circ.nchi:
        return gpu.r1cs_verify_batch_param(gens, h, nb, circ.n1, k, circ.m, pts, sc, ch, pack([c for r in recs for c in r["chi"]]), True, want_scalars)
    return gpu.r1cs_verify_batch(gens, h, nb, circ.n1, k, circ.m, pts, sc, ch, True, want_scalars)


def scalar_records(circ, mgens, nb, seed):
    rnd = random.Random(seed)
    recs = []
    for p in range(nb):
        proof, V = random_proof(rnd, circ)
        chi = None
        if circ.nchi and p < 2:                 # gadget challenges at the ends of the field
            chi = [0 if (p + j) % 2 == 0 else N - 1 for j in range(circ.nchi)] if p == 0 else [N - 1] * circ.nchi
        full, mega, ops, used = model_run(circ, mgens, proof, V, chi)
        recs.append(dict(full=full, mega=mega, ops=ops, chi=used))
    return recs


# (seed, n1, n2, m, q, nchi, profile): which scalar-assembly kernel the default options take for it
SCALAR_CIRCUITS = {
    "general np=16 dense": (1, 13, 0, 5, 40, 0, "dense"),
    "general np=128 columns": (2, 100, 0, 70, 300, 0, "columns+edge_coeff"),
    "general np=1": (3, 1, 0, 1, 1, 0, "dense"),
    "general np=4 holes": (4, 3, 0, 1, 7, 0, "holes+dups"),
    "fast np=64 m=0": (5, 64, 0, 0, 7, 0, "dense+edge_coeff"),
    "fast np=64 m=1 columns": (6, 33, 0, 1, 257, 0, "columns+edge_coeff"),
    "fast np=64 m=64": (7, 63, 0, 64, 40, 0, "dense+dups"),
    "fast np=64 n1<n": (8, 30, 20, 1, 20, 0, "sparse+dups"),
    "wave-sized np=64 m=65": (9, 64, 0, 65, 40, 0, "sparse+columns"),
    "wave-sized np=64 nchi=2": (10, 40, 10, 3, 20, 2, "dense+edge_coeff"),
    "general n1<n np=16": (11, 5, 4, 2, 12, 0, "dense"),
    "general nchi=8 np=8": (12, 3, 2, 2, 9, 8, "dense+dups"),
    "general nchi=3 holes": (13, 6, 5, 4, 30, 3, "holes+edge_coeff"),
    "no rows": (14, 3, 0, 1, 0, 0, "sparse"),
}
_RECS = {}


@pytest.mark.parametrize("large", [0, 1])
@pytest.mark.parametrize("wp", [1, 0])
@pytest.mark.parametrize("name", list(SCALAR_CIRCUITS))
def test_verifier_scalars_equal_the_model(gpu, gens, mgens, opts, name, wp, large):
    """every MSM scalar of bpgpu_r1cs_verify_batch(_param), byte for byte, against pm.Verifier.verification_msm under the same
    challenges, and mega_check against the oracle's MSM over the model's scalars; with and without the window-parallel pipeline
    (which decides who runs the inversion pass) and through the large-proof kernels (vs_large_min = 1)"""
    circ = cg.Circuit(*SCALAR_CIRCUITS[name])
    if name not in _RECS:
        _RECS[name] = scalar_records(circ, mgens, 3, 1000 + circ.seed)
    recs = _RECS[name]
    opts(verify_window_parallel=wp)
    if large:
        opts(vs_large_min=1)
    h = make(gpu, circ)
    try:
        ok, mega, full = gpu_verify(gpu, gens, circ, h, recs)
        for p, r in enumerate(recs):
            nt = len(r["full"])
            assert ints(full[nt * p:nt * (p + 1)]) == ints(r["full"]), p
            assert mega[64 * p:64 * p + 64] == r["mega"], p
            assert ok[p] == (1 if r["mega"] == IDENT else 0)
    finally:
        gpu.circuit_destroy(h)


@pytest.mark.parametrize("nb", [1, 3, 70])
def test_verifier_scalars_for_one_three_and_seventy_proofs(gpu, gens, mgens, nb):
    circ = cg.Circuit(*SCALAR_CIRCUITS["fast np=64 m=1 columns"])
    recs = scalar_records(circ, mgens, nb, 70 + nb)
    h = make(gpu, circ)
    try:
        ok, mega, full = gpu_verify(gpu, gens, circ, h, recs)
        assert full == b"".join(r["full"] for r in recs)
        assert mega == b"".join(r["mega"] for r in recs) and ok == [0] * nb
    finally:
        gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ end to end
# (seed, n1, n2, m, q, nchi, profile)
E2E = {
    "m=0": (21, 5, 0, 0, 9, 0, "sparse+dups"),
    "n=1": (22, 1, 0, 1, 2, 0, "dense"),
    "dense n=13": (23, 13, 0, 3, 40, 0, "dense"),
    "np=64 m=70": (24, 40, 0, 70, 30, 0, "sparse+holes"),
    "two-phase nchi=2": (25, 3, 3, 2, 10, 2, "dense+edge_coeff"),
    "two-phase nchi=8": (26, 2, 2, 1, 8, 8, "dense+dups"),
    "columns n=12": (27, 12, 0, 2, 40, 0, "columns+edge_coeff"),
    "two-phase numeric": (28, 4, 3, 2, 9, 0, "sparse"),
}


@pytest.fixture(scope="module")
def proofs(mgens):
    out = {}
    for name, spec in E2E.items():
        circ = cg.Circuit(*spec)
        proof, info = cg.prove(circ, mgens, spec[0])
        out[name] = (circ, proof, info["V"])
    return out


def flip(proof, V, what):
    proof, V = dict(proof), list(V)
    if what == "t_x":
        proof["t_x"] ^= 1 << 7
        if proof["t_x"] >= N:
            proof["t_x"] ^= 1 << 250
    elif V:
        V[0] = pm.pt_add(V[0], pm.G)          # one bit of the committed value
    else:
        proof["T_1"] = pm.pt_add(proof["T_1"], pm.G)
    return proof, V


@pytest.mark.parametrize("name", list(E2E))
def test_real_proofs_of_generated_circuits(gpu, gens, mgens, proofs, name):
    """pm.Prover.prove's proof of a generated circuit: the GPU accepts it with mega_check the identity; with one bit of t_x or of a
    commitment flipped it rejects it, as the model does"""
    circ, proof, V = proofs[name]
    h = make(gpu, circ)
    try:
        for what in (None, "t_x", "commitment"):
            pr, vv = (proof, V) if what is None else flip(proof, V, what)
            vf, _ = cg.verifier(circ, vv)
            accepted = vf.verify(pr, mgens)
            assert accepted == (what is None), what
            full, mega, ops, chi = model_run(circ, mgens, pr, vv)
            ok, gmega, gfull = gpu_verify(gpu, gens, circ, h, [dict(ops=ops, chi=chi)])
            assert gfull == full, what
            assert gmega == mega and (mega == IDENT) == accepted, what
            assert ok == [1 if accepted else 0], what
    finally:
        gpu.circuit_destroy(h)


def test_three_generated_circuits_in_one_combined_call(gpu, gens, mgens, proofs):
    """sum_p rho_p mega_check_p over a one-phase, a wide and a parametric circuit, valid and tampered proofs mixed"""
    rnd = random.Random(3)
    groups, want, handles = [], IDENT, []
    try:
        for name in ("dense n=13", "np=64 m=70", "two-phase nchi=2"):
            circ, proof, V = proofs[name]
            recs = []
            for what in (None, "t_x", None):
                pr, vv = (proof, V) if what is None else flip(proof, V, what)
                full, mega, ops, chi = model_run(circ, mgens, pr, vv)
                rho = rnd.randrange(1, N)
                recs.append(dict(ops=ops, chi=chi, rho=rho))
                want = o.point_add(want, o.point_mul(le(rho), mega))
            h = make(gpu, circ)
            handles.append(h)
            groups.append(dict(circuit=h, nb=len(recs), n1=circ.n1, k=(padded(circ.n) - 1).bit_length(),
                               points=b"".join(r["ops"][0] for r in recs), scalars=b"".join(r["ops"][1] for r in recs),
                               challenges=b"".join(r["ops"][2] for r in recs),
                               gadget_challenges=pack([c for r in recs for c in r["chi"]]) if circ.nchi else None,
                               rho=pack([r["rho"] for r in recs])))
        got = gpu.r1cs_verify_mixed_combined(gens, groups)
        assert got == want and got != IDENT
        assert gpu.r1cs_verify_mixed_combined(gens, [dict(g, nb=1, points=g["points"][:len(g["points"]) // 3], scalars=g["scalars"][:160],
                                                          challenges=g["challenges"][:len(g["challenges"]) // 3],
                                                          gadget_challenges=g["gadget_challenges"][:len(g["gadget_challenges"]) // 3]
                                                          if g["gadget_challenges"] else None, rho=g["rho"][:32]) for g in groups]) == IDENT
    finally:
        for h in handles:
            gpu.circuit_destroy(h)


# ------------------------------------------------------------------------------------------------ no multipliers, no rows
def test_circuits_without_multipliers_or_rows(gpu, gens, mgens, opts):
    """n = 0 (padded n = 1, k = 0: the model's answer) and q = 0 (every weight zero) on each entry point that takes a circuit"""
    rnd = random.Random(0)
    for spec in ((40, 0, 0, 2, 3, 0, "dense"), (41, 0, 0, 0, 2, 0, "sparse"), (42, 0, 0, 2, 0, 0, "sparse"), (43, 3, 0, 2, 0, 0, "sparse"),
                 (44, 0, 0, 0, 0, 0, "sparse")):
        circ = cg.Circuit(*spec)
        n, m = circ.n, circ.m
        h = make(gpu, circ)
        try:
            check_flatten(gpu, circ, h, [rnd.randrange(N), 1, N - 1])
            # the verifier
            recs = scalar_records(circ, mgens, 2, spec[0])
            for large in (0, 1):
                if large:
                    opts(vs_large_min=1)
                ok, mega, full = gpu_verify(gpu, gens, circ, h, recs)
                assert full == b"".join(r["full"] for r in recs), (spec, large)
                assert mega == b"".join(r["mega"] for r in recs), (spec, large)
            # the prover
            y, z, x = rnd.randrange(1, N), rnd.randrange(N), rnd.randrange(N)
            wit = random_witness(rnd, n)
            t, wv, ses = gpu.r1cs_prover_polys(h, 1, n, m, le(y), le(pow(y, -1, N)), le(z), *(pack(wit[k]) for k in ("aL", "aR", "aO", "sL", "sR")))
            lv, rv = gpu.r1cs_prover_eval(ses, 1, padded(n), le(x))
            gpu.prover_destroy(ses)
            weights = cg.model_weights(circ, z)
            want_t, want_l, want_r = model_polys(circ, weights, y, x, wit)
            assert (ints(t), ints(wv), ints(lv), ints(rv)) == (want_t, weights[3], want_l, want_r), spec
        finally:
            gpu.circuit_destroy(h)
    # a real proof of a circuit without multipliers: accepted
    circ = cg.Circuit(45, 0, 0, 2, 3, 0, "dense")
    proof, info = cg.prove(circ, mgens, 45)
    vf, _ = cg.verifier(circ, info["V"])
    assert vf.verify(proof, mgens)
    full, mega, ops, chi = model_run(circ, mgens, proof, info["V"])
    h = make(gpu, circ)
    try:
        ok, gmega, gfull = gpu_verify(gpu, gens, circ, h, [dict(ops=ops, chi=chi)])
        assert (ok, gmega, gfull) == ([1], IDENT, full)
    finally:
        gpu.circuit_destroy(h)
