"""bpgpu_r1cs_prove_fs2 / _dev: a two-phase prover in ONE call, its gadget a bpgpu_witness gate program evaluated on the device.  The
shuffle (k = 2, 4, 9) and the composite gadget of tests/witness_cases.py, 1 and 5 provers, explicit blinding vectors and keys: the
bytes of pm.Prover.prove under the replay RNG, the bytes of the _begin / _finish pair fed the host-evaluated witness, accepted by
bpgpu_r1cs_verify_batch_wire2."""
import random

import pytest

import mpc_dealer as md
import oracle_lib as o
import witness_cases as wc
from prove_fs_cases import Replay, label, lg_padded

pytestmark = pytest.mark.gpu
pm = wc.pm
N = wc.N
le, mont, cut = md.le, md.mont, md.cut
CAP = 16
LABEL = wc.SHUFFLE_LABEL
NAMES = ("shuffle2", "shuffle4", "shuffle9", "composite")


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


class ModelGens:
    """the model's BulletproofGens interface over the oracle's generator chain"""

    def __init__(self, cap):
        self.gens_capacity = cap
        self._g = [pm.b2p(b) for b in cut(o.gens("G", cap), 64)]
        self._h = [pm.b2p(b) for b in cut(o.gens("H", cap), 64)]

    def G(self, n, share=0):
        return self._g[:n]

    def H(self, n, share=0):
        return self._h[:n]


@pytest.fixture(scope="module")
def mgens():
    return ModelGens(CAP)


def ark(values):
    return b"".join(map(mont, values))


def _expand(key, cnt):
    return tuple([int.from_bytes(b, "little") for b in cut(o.blind_vector(key, side, cnt), 32)] if cnt else [] for side in (0, 1))


_records = {}


def record(mgens, name, p):
    """prover p of a case under its own transcript label, values and blindings: the operands of the call for this prover and the
    model's outputs (computed once, left unchanged: the model takes 0.5-3 s per proof).  The gadget's challenge is the transcript's,
    not the case's.  The explicit blinding vectors are the expansions of the two keys, so that one model proof serves both sources."""
    if (name, p) in _records:
        return _records[(name, p)]
    case = wc.case(name)
    prog = case.prog
    n, n1 = prog.n, prog.phase1
    n2 = n - n1
    v, inputs, _ = case.prover(p)
    rnd = random.Random(9000 + 10 * p + 100 * NAMES.index(name))
    vb = [rnd.randrange(N) for _ in range(prog.m)]
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(label(p)))
    committed = [pv.commit(x, b) for x, b in zip(v, vb)]
    case.gadget(pv, [c[1] for c in committed], v, inputs)
    q1, state_in = len(pv.constraints), pv.transcript.state
    drawn = []
    draw = pv.challenge_scalar
    pv.challenge_scalar = lambda lab: drawn.append(draw(lab)) or drawn[-1]
    bl1 = [rnd.randrange(N) for _ in range(3)]
    key1, key2 = (bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(2))
    bl2 = [rnd.randrange(N) for _ in range(3)]
    tb = [rnd.randrange(N) for _ in range(5)]
    (sL1, sR1), (sL2, sR2) = _expand(key1, n1), _expand(key2, n2)
    trace = {}
    rng = Replay(bl1 + sL1 + sR1 + bl2 + sL2 + sR2 + tb)
    proof = pv.prove(mgens, rng, trace=trace)
    assert not rng.values and len(drawn) == 1 and len(pv.a_L) == n
    # the helper's evaluator on the transcript's challenge is the model's witness
    assert tuple(prog.evaluate(v, inputs, (drawn[0],))) == (pv.a_L, pv.a_R, pv.a_O)
    order = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6")
    points = b"".join(pm.p2b(proof[k]) for k in order) + b"".join(map(pm.p2b, proof["L_vec"])) + b"".join(map(pm.p2b, proof["R_vec"]))
    rec = dict(
        state_in=state_in, v=ark(v), inputs=ark(x for pair in inputs for x in pair), v_blinding=ark(vb), blindings=ark(bl1 + bl2 + tb),
        s_L=ark(sL1 + sL2), s_R=ark(sR1 + sR2), keys=key1 + key2, bl1=ark(bl1), bl2=ark(bl2 + tb), key1=key1, key2=key2,
        s_L1=ark(sL1), s_R1=ark(sR1), s_L2=ark(sL2), s_R2=ark(sR2), planes=tuple(ark(x) for x in (pv.a_L, pv.a_R, pv.a_O)),
        witness=(pv.a_L, pv.a_R, pv.a_O), chi=le(drawn[0]), constraints=pv.constraints, q1=q1, chi_int=drawn[0],
        V=b"".join(pm.point_compress(c[0]) for c in committed), init=pm.Transcript(label(p)).state,
        points=points, scalars=b"".join(le(proof[k]) for k in ("t_x", "t_x_blinding", "e_blinding", "a", "b")),
        challenges=b"".join(le(trace[k]) for k in "yzuxw") + b"".join(le(u) for u, _ in trace["ipp"]),
        state_out=pv.transcript.state, wire=pm.r1cs_proof_to_bytes(proof))
    _records[(name, p)] = rec
    return rec


def operands(recs, keys):
    cat = lambda k: b"".join(r[k] for r in recs)      # noqa: E731
    kw = dict(states=cat("state_in"), v=cat("v"), inputs=cat("inputs") or None, v_blinding=cat("v_blinding"), blindings=cat("blindings"))
    if keys:
        kw["vector_keys"] = cat("keys")
    else:
        kw["s_L"], kw["s_R"] = cat("s_L"), cat("s_R")
    return kw


def handles(gpu, name, rec):
    case = wc.case(name)
    q, nchi, rp, kd, ix, cf = wc.circuit_from(rec["constraints"], rec["q1"], (rec["chi_int"],), 1)
    return gpu.circuit_create_param(q, 1, rp, kd, ix, cf, case.prog.n, case.prog.m), gpu.witness_create(*case.prog.create_args())


def two_calls(gpu, gens, circ, case, recs, keys):
    """the existing pair, fed the witness the host evaluated"""
    nb, n, n1 = len(recs), case.prog.n, case.prog.phase1
    cat = lambda k: b"".join(r[k] for r in recs)      # noqa: E731
    part = lambda k, lo, hi: b"".join(r["planes"][k][32 * lo:32 * hi] for r in recs)      # noqa: E731
    first = dict(states=cat("state_in"), blindings=cat("bl1"))
    if n1:
        first.update(a_L=part(0, 0, n1), a_R=part(1, 0, n1), a_O=part(2, 0, n1))
        first.update(dict(vector_keys=cat("key1")) if keys else dict(s_L=cat("s_L1"), s_R=cat("s_R1")))
    sess, _, chi, _ = gpu.r1cs_prove_fs2_begin(gens, circ, nb, n1, gadget_label=LABEL, **first)
    assert chi == cat("chi")
    second = dict(a_L=part(0, n1, n), a_R=part(1, n1, n), a_O=part(2, n1, n), blindings=cat("bl2"), v_blinding=cat("v_blinding"))
    second.update(dict(vector_keys=cat("key2")) if keys else dict(s_L=cat("s_L2"), s_R=cat("s_R2")))
    return gpu.r1cs_prove_fs2_finish(gens, circ, sess, nb, n, case.prog.m, **second)


@pytest.mark.parametrize("nb", (1, 5))
@pytest.mark.parametrize("keys", (False, True), ids=("explicit", "keys"))
@pytest.mark.parametrize("name", NAMES)
def test_one_call_equals_the_model_and_the_two_calls(gpu, gens, mgens, name, keys, nb):
    case = wc.case(name)
    n, m, n1 = case.prog.n, case.prog.m, case.prog.phase1
    k = lg_padded(n)
    plen = 1 + 14 * 32 + (2 * k + 2) * 32
    recs = [record(mgens, name, p) for p in range(nb)]
    cat = lambda key: b"".join(r[key] for r in recs)      # noqa: E731
    circ, w = handles(gpu, name, recs[0])
    try:
        for route in (0, 1, 2):
            gpu.set_option("witness_route", route)
            pts, sc, wire, ch, so, chi, planes = gpu.r1cs_prove_fs2(gens, circ, w, nb, n, m, gadget_label=LABEL, want_witness=True,
                                                                    **operands(recs, keys))
            # the model's bytes
            assert chi == cat("chi") and planes == tuple(b"".join(r["planes"][i] for r in recs) for i in range(3)), route
            assert (pts, sc, wire, ch, so) == (cat("points"), cat("scalars"), cat("wire"), cat("challenges"), cat("state_out")), route
        gpu.set_option("witness_route", 0)
        # ... which are the bytes of the two calls around a host that evaluates the gadget
        assert two_calls(gpu, gens, circ, case, recs, keys) == (pts, sc, wire, ch, so)
        assert len(wire) == nb * plen and wire[0] == 1
        assert gpu.r1cs_verify_batch_wire2(gens, circ, nb, n1, plen, LABEL, wire, cat("V"), cat("init")) == [1] * nb
        # the witness it hands back satisfies the circuit on the challenge it hands back
        ok, row, gate, _ = gpu.r1cs_constraints_satisfied(circ, nb, len(recs[0]["constraints"]), *planes, v=cat("v"), gadget_challenges=chi)
        assert ok == [1] * nb and row == [-1] * nb and gate == [-1] * nb
    finally:
        gpu.set_option("witness_route", 0)
        gpu.witness_destroy(w)
        gpu.circuit_destroy(circ)


def test_dev_form_is_enqueued_without_a_synchronise(gpu, gens, mgens):
    """every operand and result in device memory; nothing is waited for between the call and the downloads; a bad limb raises the flag"""
    name, keys, nb = "composite", True, 5
    case = wc.case(name)
    n, m = case.prog.n, case.prog.m
    k = lg_padded(n)
    recs = [record(mgens, name, p) for p in range(nb)]
    cat = lambda key: b"".join(r[key] for r in recs)      # noqa: E731
    ops = operands(recs, keys)
    sizes = dict(points=64 * nb * (11 + 2 * k), scalars=160 * nb, wire=nb * (1 + 14 * 32 + (2 * k + 2) * 32), challenges=32 * nb * (5 + k),
                 state_out=32 * nb, chi=32 * nb)
    circ, w = handles(gpu, name, recs[0])
    bufs = []
    try:
        d = {key: gpu.to_device(val) for key, val in ops.items() if val is not None}
        out = {key: gpu.malloc(size) for key, size in sizes.items()}
        planes = [gpu.malloc(32 * nb * n) for _ in range(3)]
        bufs = list(d.values()) + list(out.values()) + planes

        def run():
            gpu.r1cs_prove_fs2_dev(gens, circ, w, nb, d["states"], LABEL, d["blindings"], out["points"], out["scalars"], d_v=d["v"],
                                   d_inputs=d.get("inputs"), d_v_blinding=d["v_blinding"], d_vector_keys=d["vector_keys"], d_wire=out["wire"],
                                   d_ch=out["challenges"], d_states_out=out["state_out"], d_chi=out["chi"], d_a_L=planes[0], d_a_R=planes[1],
                                   d_a_O=planes[2])
        run()
        for key, size in sizes.items():
            assert gpu.download(out[key], size) == cat(key), key
        assert tuple(gpu.download(p, 32 * nb * n) for p in planes) == tuple(b"".join(r["planes"][i] for r in recs) for i in range(3))
        assert gpu.input_flag() == 0
        # the optional results left out
        gpu.r1cs_prove_fs2_dev(gens, circ, w, nb, d["states"], LABEL, d["blindings"], out["points"], out["scalars"], d_v=d["v"],
                               d_inputs=d.get("inputs"), d_v_blinding=d["v_blinding"], d_vector_keys=d["vector_keys"])
        assert gpu.download(out["points"], sizes["points"]) == cat("points") and gpu.input_flag() == 0
        # a committed value of prover 2 := the group order
        bad = ops["v"][:32 * (2 * m + 1)] + N.to_bytes(32, "little") + ops["v"][32 * (2 * m + 2):]
        gpu.upload(d["v"], bad)
        run()
        assert gpu.input_flag() == 1
        gpu.upload(d["v"], ops["v"])
        run()
        assert gpu.input_flag() == 0 and gpu.download(out["wire"], sizes["wire"]) == cat("wire")
    finally:
        for b in bufs:
            gpu.free(b)
        gpu.witness_destroy(w)
        gpu.circuit_destroy(circ)


def test_refusals_leave_nothing_behind(gpu, gens, mgens):
    import mpc_bulletproof_amd as mm
    E = mm.lib
    name, keys = "composite", False
    case = wc.case(name)
    n, m = case.prog.n, case.prog.m
    rec = record(mgens, name, 0)
    ops = operands([rec], keys)
    circ, w = handles(gpu, name, rec)
    other = wc.case("shuffle4")
    w_other = gpu.witness_create(*other.prog.create_args())
    small = gpu.gens_create(o.gens("G", 8), o.gens("H", 8), o.generator(), o.generator(), 8)

    def code(g=gens, c=circ, prog=w, **over):
        try:
            gpu.r1cs_prove_fs2(g, c, prog, 1, n, m, gadget_label=LABEL, **dict(ops, **over))
        except E.BpGpuError as e:
            return e.code
        return 0
    try:
        assert code(prog=w_other) == E.E_ARG                                   # a program that is not the circuit's
        assert code(prog=None) == E.E_ARG and code(c=None) == E.E_ARG and code(g=None) == E.E_ARG
        for key in ("states", "v", "inputs", "v_blinding", "blindings"):
            assert code(**{key: None}) == E.E_ARG, key
        assert code(s_L=None) == E.E_ARG and code(s_L=None, s_R=None) == E.E_ARG and code(vector_keys=rec["keys"]) == E.E_ARG
        assert code(g=small) == E.E_GENS
        gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, 0, 2))
        try:
            assert code() == E.E_ARG
        finally:
            gpu._ck(E._lib.bpgpu_set_shard(gpu.ctx, 0, 1))
        # a launched call that fails on an operand
        assert code(v=N.to_bytes(32, "little") + ops["v"][32:]) == E.E_ARG
        assert code(blindings=ops["blindings"][:-32] + N.to_bytes(32, "little")) == E.E_ARG
        none = [None] * 18
        assert E._lib.bpgpu_r1cs_prove_fs2(gpu.ctx, gens, circ, w, 0, *none) == 0          # nb == 0
        # no session, no pool memory, no flag is left behind: the context proves as before, in one call and in two
        out = gpu.r1cs_prove_fs2(gens, circ, w, 1, n, m, gadget_label=LABEL, **ops)
        assert out[:5] == (rec["points"], rec["scalars"], rec["wire"], rec["challenges"], rec["state_out"])
        assert two_calls(gpu, gens, circ, case, [rec], keys) == out[:5]
    finally:
        gpu.gens_destroy(small)
        gpu.witness_destroy(w_other)
        gpu.witness_destroy(w)
        gpu.circuit_destroy(circ)
