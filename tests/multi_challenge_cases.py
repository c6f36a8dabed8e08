"""Circuits whose randomized phase draws SEVERAL gadget challenges, each under its own label (two composed gadgets: two shuffles, a
shuffle next to a Horner check), and what the device-transcript entry points must return for them, from the Python model
(oracle/pymodel.py through tests/circuit_gen.py): generated circuits affine in 2, 3 and 8 challenges installed so that draw j uses label
j, the model's proofs under a replay RNG, the model verifier's verdicts and challenges, and a gate program of two shuffles side by
side.  The reference of tests/test_multi_challenge_cases.py and tests/test_gpu_multi_challenge.py: computed once per record and left
unchanged.  No GPU needed."""
import random

import circuit_gen as cg
import mpc_dealer as md
import oracle_lib as o
import witness_cases as wc
from prove_fs_cases import Replay, label, lg_padded      # noqa: F401  (re-exported for the tests)

pm = cg.pm
N = pm.N
le, mont, cut = md.le, md.mont, md.cut

# (n1, n2, m, q, nchi, profile): k = 0 with no phase-1 multipliers and no commitments; the shape of the refusal test's two_chi; pad = 3
# with duplicates and empty rows; every challenge the handle allows, m = 17 (the block-wide <wV, v_blinding>), pad = 0
SHAPES = [(0, 1, 0, 2, 2, "dense"), (1, 1, 1, 4, 2, "sparse"), (2, 3, 2, 9, 3, "dups+holes"), (3, 5, 17, 20, 8, "sparse")]
# a lane per proof in blocks of 64: 65 puts the last proof alone in a second wave.  The model proves (and verifies) these provers of a
# batch; the others of the 65 are prover 0's witness and blindings under their own transcript labels
BATCHES = (1, 3, 65)
MODEL_PROVERS = {1: (0,), 3: (0, 1, 2), 65: (0, 63, 64)}
CAP = 16


def labels_for(nchi):
    """nchi distinct labels: short ones, one that fills all 32 bytes (no padding), and two that differ in the last byte only"""
    base = [b"first gadget", b"second gadget: a 32-byte label..", b"horner x", b"horner y", b"g4", b"g5", b"g6", b"g7"]
    assert len(base[1]) == 32 and len(set(base)) == 8
    return base[:nchi]


class Circuit(cg.Circuit):
    """cg.Circuit whose randomized phase draws challenge j under labels[j] (cg.Circuit draws all of them under cg.CHI_LABEL)"""

    def __init__(self, seed, n1, n2, m, q, nchi, profile, labels=None):
        super().__init__(seed, n1, n2, m, q, nchi, profile)
        self.labels = list(labels) if labels is not None else labels_for(nchi)
        assert len(self.labels) == nchi

    def install(self, cs, rng=None, commitments=None, chi=None, labels=None):
        """as cg.Circuit.install; labels replaces the circuit's own (a verifier that holds them in another order)"""
        labels = self.labels if labels is None else list(labels)
        prover = isinstance(cs, pm.Prover)
        info = {"V": [], "chi": None}
        for i in range(self.m):
            if prover:
                info["V"].append(cs.commit(self.v[i], rng.scalar())[0])
            else:
                cs.commit(commitments[i])
                info["V"].append(commitments[i])

        def multipliers(lo, hi):
            for i in range(lo, hi):
                cs.allocate_multiplier((self.a_L[i], self.a_R[i]) if prover else None)

        multipliers(0, self.n1)
        for row in self.rows[:self.q1]:
            cs.constrain(pm.lc(*row))

        def phase2(cs2):
            drawn = [cs2.challenge_scalar(labels[j]) for j in range(self.nchi)]
            info["chi"] = list(chi) if chi is not None else drawn
            multipliers(self.n1, self.n)
            for row in self.rows[self.q1:]:
                cs2.constrain(pm.lc(*[(var, cg.coeff_at(c, info["chi"])) for var, c in row]))
        cs.specify_randomized_constraints(phase2)
        return info


_circuits = {}


def circuit(shape):
    """the shape's circuit (built once).  (1, 1, 1, 4, 2, sparse) is the generator's seed-8 circuit of the refusal test"""
    if shape not in _circuits:
        n1, n2, m, q, nchi, profile = shape
        seed = 8 if shape == SHAPES[1] else 800 + 10 * n1 + n2
        _circuits[shape] = Circuit(seed, n1, n2, m, q, nchi, profile)
    return _circuits[shape]


class ModelGens:
    """the model's BulletproofGens interface over the oracle's generator chain"""

    def __init__(self, cap=CAP):
        self.gens_capacity = cap
        self._g = [pm.b2p(b) for b in cut(o.gens("G", cap), 64)]
        self._h = [pm.b2p(b) for b in cut(o.gens("H", cap), 64)]

    def G(self, n, share=0):
        return self._g[:n]

    def H(self, n, share=0):
        return self._h[:n]


_mgens = []


def mgens():
    if not _mgens:
        _mgens.append(ModelGens())
    return _mgens[0]


def ark(values):
    return b"".join(map(mont, values))


def _expand(key, cnt):
    return tuple([int.from_bytes(b, "little") for b in cut(o.blind_vector(key, side, cnt), 32)] if cnt else [] for side in (0, 1))


def state_after_commitments(p, V):
    """the chain on entry to Prover::prove for transcript label(p) and the commitments V: Prover::new, then Prover::commit each"""
    tr = pm.Transcript(label(p))
    tr.r1cs_domain_sep()
    for pt in V:
        tr.append_point(b"V", pt)
    return tr.state


def verify_model(circ, p, V, proof, labels=None):
    """pm.Verifier.verify of a proof under transcript label(p) -> (accepted, the verifier's challenges y z u x w r u_1..u_k as the
    device returns them, its gadget challenges)"""
    vf = pm.Verifier(pm.PedersenGens(), pm.Transcript(label(p)))
    info = circ.install(vf, commitments=V, labels=labels)
    trace = {}
    ok = bool(vf.verify(proof, mgens(), trace=trace))
    ch = b"".join(le(trace[k]) for k in "yzuxwr") + b"".join(le(u) for u in trace["ipp_u"])
    return ok, ch, b"".join(le(x) for x in info["chi"])


_records = {}


def record(shape, p):
    """Prover p of a shape's batch: the operands of _begin / _finish for it (ark form where the ABI takes it; the explicit blinding
    vectors are the expansions of the two keys, so that one model proof serves both sources), the model's proof, the bytes both calls
    and the verifiers are expected to return, and the model verifier's verdict and challenges.  Computed once."""
    if (shape, p) in _records:
        return _records[(shape, p)]
    circ = circuit(shape)
    rnd = random.Random(8000 + 1000 * SHAPES.index(shape) + p)
    n1, n2, n, m = circ.n1, circ.n2, circ.n, circ.m
    vb = [rnd.randrange(N) for _ in range(m)]
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(label(p)))
    info = circ.install(pv, rng=Replay(vb))
    state_in = pv.transcript.state
    assert state_in == state_after_commitments(p, info["V"])
    bl1 = [rnd.randrange(N) for _ in range(3)]
    key1, key2 = (bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(2))
    bl2 = [rnd.randrange(N) for _ in range(3)]
    tb = [rnd.randrange(N) for _ in range(5)]
    (sL1, sR1), (sL2, sR2) = _expand(key1, n1), _expand(key2, n2)
    trace = {}
    rng = Replay(bl1 + sL1 + sR1 + bl2 + sL2 + sR2 + tb)
    proof = pv.prove(mgens(), rng, trace=trace)
    assert not rng.values and len(info["chi"]) == circ.nchi
    order = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6")
    points = b"".join(pm.p2b(proof[k]) for k in order) + b"".join(map(pm.p2b, proof["L_vec"])) + b"".join(map(pm.p2b, proof["R_vec"]))
    # the chain after the last gadget challenge, replayed: "m", A_I1 A_O1 S1, the 2-phase separator, draw j under label j
    tr = pm.Transcript(b"")
    tr.state = state_in
    tr.append_u64(b"m", m)
    for lab in ("A_I1", "A_O1", "S1"):
        tr.append_point(lab.encode(), proof[lab])
    tr.r1cs_2phase_domain_sep()
    assert [tr.challenge_scalar(lab) for lab in circ.labels] == info["chi"]
    aO = [circ.a_L[i] * circ.a_R[i] for i in range(n)]
    accepted, vch, vchi = verify_model(circ, p, info["V"], proof)
    rec = dict(
        p=p, state_in=state_in, init=pm.Transcript(label(p)).state, key1=key1, key2=key2, v_blinding=ark(vb), bl1=ark(bl1), bl2=ark(bl2 + tb),
        a_L1=ark(circ.a_L[:n1]), a_R1=ark(circ.a_R[:n1]), a_O1=ark(aO[:n1]), s_L1=ark(sL1), s_R1=ark(sR1),
        a_L2=ark(circ.a_L[n1:n]), a_R2=ark(circ.a_R[n1:n]), a_O2=ark(aO[n1:n]), s_L2=ark(sL2), s_R2=ark(sR2),
        proof=proof, V=info["V"], V_xy=b"".join(pm.p2b(v) for v in info["V"]), V_compressed=b"".join(pm.point_compress(v) for v in info["V"]),
        chi=b"".join(le(x) for x in info["chi"]), commitments=points[:192], state_mid=tr.state,
        points=points, scalars=b"".join(le(proof[k]) for k in ("t_x", "t_x_blinding", "e_blinding", "a", "b")),
        challenges=b"".join(le(trace[k]) for k in "yzuxw") + b"".join(le(u) for u, _ in trace["ipp"]),
        state_out=pv.transcript.state, wire=pm.r1cs_proof_to_bytes(proof),
        accepted=accepted, verifier_challenges=vch, verifier_chi=vchi)
    _records[(shape, p)] = rec
    return rec


def batch(shape, nb):
    """nb provers of a shape: the model's records where it proves, copies of prover 0 under their own transcript labels elsewhere
    (no model outputs: whoever needs their proofs makes them on the device) -> (records, the provers the model covers)"""
    r0 = record(shape, 0)
    recs = []
    for p in range(nb):
        if p in MODEL_PROVERS[nb]:
            recs.append(record(shape, p))
        else:
            r = {k: r0[k] for k in ("key1", "key2", "v_blinding", "bl1", "bl2", "a_L1", "a_R1", "a_O1", "s_L1", "s_R1", "a_L2", "a_R2", "a_O2",
                                    "s_L2", "s_R2", "V", "V_xy", "V_compressed")}
            r.update(p=p, init=pm.Transcript(label(p)).state, state_in=state_after_commitments(p, r0["V"]))
            recs.append(r)
    return recs, MODEL_PROVERS[nb]


def begin_operands(recs, keys, n1):
    """the keyword operands of BpGpu.r1cs_prove_fs2_begin for a batch of records"""
    cat = lambda k: b"".join(r[k] for r in recs)      # noqa: E731
    kw = dict(states=cat("state_in"), blindings=cat("bl1"))
    if n1:
        kw.update(a_L=cat("a_L1"), a_R=cat("a_R1"), a_O=cat("a_O1"))
        kw.update(dict(vector_keys=cat("key1")) if keys else dict(s_L=cat("s_L1"), s_R=cat("s_R1")))
    return kw


def finish_operands(recs, keys):
    """... and of BpGpu.r1cs_prove_fs2_finish"""
    cat = lambda k: b"".join(r[k] for r in recs)      # noqa: E731
    kw = dict(a_L=cat("a_L2"), a_R=cat("a_R2"), a_O=cat("a_O2"), blindings=cat("bl2"), v_blinding=cat("v_blinding") or None)
    kw.update(dict(vector_keys=cat("key2")) if keys else dict(s_L=cat("s_L2"), s_R=cat("s_R2")))
    return kw


def with_commitments(points, recs, k):
    """the verifier's operand layout: V_0..V_{m-1} inserted after the six A / S points of each proof"""
    nvar, out = 11 + 2 * k, b""
    for p, r in enumerate(recs):
        pp = points[64 * nvar * p:64 * nvar * (p + 1)]
        out += pp[:6 * 64] + r["V_xy"] + pp[6 * 64:]
    return out


# ---- two shuffles side by side: a gate program with nchi = 2 ------------------------------------------------------------------------
SHUFFLE_KS = (2, 3)
SHUFFLE_LABELS = [b"shuffle challenge", b"second shuffle challenge"]


def two_shuffles_program():
    """tests/r1cs.rs:36-61 twice, over V_0..V_3 (k = 2) and V_4..V_9 (k = 3): every gate in phase 2, the first shuffle's chains read
    chi_1, the second's chi_2"""
    prog = wc.Program(2 * sum(SHUFFLE_KS), nchi=2)
    prog.end_phase1()
    base, outs = 0, []
    for j, k in enumerate(SHUFFLE_KS):
        mz = (wc.ONE, 0, tuple(N - 1 if t == j + 1 else None for t in range(3)))
        for side in (base, base + k):
            last = prog.mul([(wc.V, side + k - 1, 1), mz], [(wc.V, side + k - 2, 1), mz])
            for i in range(k - 3, -1, -1):
                last = prog.mul([(wc.O, last, 1)], [(wc.V, side + i, 1), mz])
            outs.append(last)
        base += 2 * k
    return prog, outs


def two_shuffles_rows(prog, outs):
    """the circuit the program's witness satisfies, as circuit_gen rows (all of phase 2): a_L[i] = left row, a_R[i] = right row of
    every gate, and per shuffle the two chains' products are equal"""
    var = {wc.L: "L", wc.R: "R", wc.O: "O", wc.V: "V"}
    rows = []
    for i, (_, _, left, right) in enumerate(prog.gates):
        for side, row in (("L", left), ("R", right)):
            terms = [((side, i), (N - 1, None, None))]
            for kind, idx, c in row:
                terms.append((cg.ONE if kind == wc.ONE else (var[kind], idx), prog.parts(c)))
            rows.append(terms)
    for a, b in zip(outs[0::2], outs[1::2]):
        rows.append([(("O", a), (1, None, None)), (("O", b), (N - 1, None, None))])
    return rows


def two_shuffles_values(p, wrong=False):
    """prover p's committed values x_1 | y_1 | x_2 | y_2 (y a permutation of x); wrong: y_2's first value moved by one"""
    rnd = random.Random(4200 + p)
    v = []
    for k in SHUFFLE_KS:
        v += wc._shuffle_values(rnd, k)
    if wrong:
        v[2 * SHUFFLE_KS[0] + SHUFFLE_KS[1]] += 1
    return v


def two_shuffles_prover(p, wrong=False):
    """the operands of bpgpu_r1cs_prove_fs2 / _prove_values for prover p (the blinding vectors from two keys), and what the verifier
    needs: the commitments and the transcript's initial state"""
    rnd = random.Random(4300 + p)
    prog, _ = two_shuffles_program()
    v = two_shuffles_values(p, wrong)
    vb = [rnd.randrange(N) for _ in range(prog.m)]
    pg = pm.PedersenGens()
    V = [pg.commit(x, b) for x, b in zip(v, vb)]
    key1, key2 = (bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(2))
    sL, sR = _expand(key2, prog.n)
    bl = [rnd.randrange(N) for _ in range(11)]
    return dict(p=p, v_int=v, v=ark(v), v_blinding=ark(vb), V=V, V_xy=b"".join(pm.p2b(x) for x in V),
                V_compressed=b"".join(pm.point_compress(x) for x in V), init=pm.Transcript(label(p)).state,
                state_in=state_after_commitments(p, V), keys=key1 + key2, key1=key1, key2=key2, s_L=ark(sL), s_R=ark(sR),
                blindings=ark(bl), bl1=ark(bl[:3]), bl2=ark(bl[3:]))
