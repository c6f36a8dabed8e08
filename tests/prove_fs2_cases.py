"""Inputs and expected outputs of bpgpu_r1cs_prove_fs2_begin / _finish from the Python model: pm.Prover.prove on a generated two-phase
circuit with one gadget challenge (tests/circuit_gen.py), driven by a replay RNG that hands the model the blindings the GPU calls
get.  No GPU needed."""
import random

import circuit_gen as cg
import mpc_dealer as md
import oracle_lib as o
from prove_fs_cases import Replay, label, lg_padded      # noqa: F401  (re-exported for the tests)

pm = cg.pm
N = pm.N
le, mont = md.le, md.mont

# (n1, n2, m, q, profile): the smallest shapes that reach every branch -- k = 0 with no phase-1 multipliers and no commitments; pad = 3;
# m = 17, the block-wide <wV, v_blinding>; pad = 0; k = 4
SHAPES = [(0, 1, 0, 2, "dense"), (0, 2, 2, 5, "sparse"), (1, 1, 1, 4, "sparse"), (2, 3, 2, 9, "dups+holes"), (3, 5, 17, 20, "sparse"),
          (4, 4, 1, 16, "columns+edge_coeff"), (6, 7, 3, 30, "dense")]


def circuit(shape):
    n1, n2, m, q, profile = shape
    return cg.Circuit(700 + 10 * n1 + n2, n1, n2, m, q, 1, profile)


def _vectors(rnd, key, vkeys, cnt):
    """s_L, s_R of one phase: drawn, or the expansion of the phase's key (index from 0)"""
    if vkeys:
        return ([int.from_bytes(b, "little") for b in md.cut(o.blind_vector(key, 0, cnt), 32)] if cnt else [],
                [int.from_bytes(b, "little") for b in md.cut(o.blind_vector(key, 1, cnt), 32)] if cnt else [])
    return [rnd.randrange(N) for _ in range(cnt)], [rnd.randrange(N) for _ in range(cnt)]


def model_proof(circ, mgens, p, vkeys, seed):
    """proof p of a batch; vkeys = (phase 1 from a key, phase 2 from a key).  The record holds the operands of both calls for this
    proof (ark form where the ABI takes it), the model's proof and the bytes both calls are expected to return."""
    rnd = random.Random(seed * 1000 + p * 4 + 2 * int(vkeys[0]) + int(vkeys[1]))
    n1, n2, n, m = circ.n1, circ.n2, circ.n, circ.m
    vb = [rnd.randrange(N) for _ in range(m)]
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(label(p)))
    info = circ.install(pv, rng=Replay(vb))
    state_in = pv.transcript.state
    bl1 = [rnd.randrange(N) for _ in range(3)]
    key1 = bytes(rnd.getrandbits(8) for _ in range(32))
    sL1, sR1 = _vectors(rnd, key1, vkeys[0], n1)
    bl2 = [rnd.randrange(N) for _ in range(3)]
    key2 = bytes(rnd.getrandbits(8) for _ in range(32))
    sL2, sR2 = _vectors(rnd, key2, vkeys[1], n2)
    tb = [rnd.randrange(N) for _ in range(5)]
    trace = {}
    rng = Replay(bl1 + sL1 + sR1 + bl2 + sL2 + sR2 + tb)
    proof = pv.prove(mgens, rng, trace=trace)
    assert not rng.values and len(info["chi"]) == 1
    order = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6")
    points = b"".join(pm.p2b(proof[k]) for k in order) + b"".join(map(pm.p2b, proof["L_vec"])) + b"".join(map(pm.p2b, proof["R_vec"]))
    scalars = b"".join(le(proof[k]) for k in ("t_x", "t_x_blinding", "e_blinding", "a", "b"))
    ch = b"".join(le(trace[k]) for k in "yzuxw") + b"".join(le(u) for u, _ in trace["ipp"])
    # the chain after the gadget challenge, replayed: "m", A_I1 A_O1 S1, the 2-phase separator, the challenge
    tr = pm.Transcript(b"")
    tr.state = state_in
    tr.append_u64(b"m", m)
    for lab, k in ((b"A_I1", "A_I1"), (b"A_O1", "A_O1"), (b"S1", "S1")):
        tr.append_point(lab, proof[k])
    tr.r1cs_2phase_domain_sep()
    assert tr.challenge_scalar(cg.CHI_LABEL) == info["chi"][0]
    aO = [circ.a_L[i] * circ.a_R[i] for i in range(n)]
    ark = lambda v: b"".join(map(mont, v))      # noqa: E731
    return dict(
        state_in=state_in, key1=key1, key2=key2, v_blinding=ark(vb), bl1=ark(bl1), bl2=ark(bl2 + tb),
        a_L1=ark(circ.a_L[:n1]), a_R1=ark(circ.a_R[:n1]), a_O1=ark(aO[:n1]), s_L1=ark(sL1), s_R1=ark(sR1),
        a_L2=ark(circ.a_L[n1:n]), a_R2=ark(circ.a_R[n1:n]), a_O2=ark(aO[n1:n]), s_L2=ark(sL2), s_R2=ark(sR2),
        proof=proof, V=info["V"], trace=trace, chi=le(info["chi"][0]), commitments=points[:192], state_mid=tr.state,
        points=points, scalars=scalars, challenges=ch, state_out=pv.transcript.state, wire=pm.r1cs_proof_to_bytes(proof))


def begin_operands(recs, vkeys, n1):
    """the keyword operands of BpGpu.r1cs_prove_fs2_begin for a batch of records"""
    cat = lambda k: b"".join(r[k] for r in recs)      # noqa: E731
    kw = dict(states=cat("state_in"), blindings=cat("bl1"))
    if n1:
        kw.update(a_L=cat("a_L1"), a_R=cat("a_R1"), a_O=cat("a_O1"))
        if vkeys[0]:
            kw["vector_keys"] = cat("key1")
        else:
            kw["s_L"], kw["s_R"] = cat("s_L1"), cat("s_R1")
    return kw


def finish_operands(recs, vkeys):
    """... and of BpGpu.r1cs_prove_fs2_finish"""
    cat = lambda k: b"".join(r[k] for r in recs)      # noqa: E731
    kw = dict(a_L=cat("a_L2"), a_R=cat("a_R2"), a_O=cat("a_O2"), blindings=cat("bl2"), v_blinding=cat("v_blinding") or None)
    if vkeys[1]:
        kw["vector_keys"] = cat("key2")
    else:
        kw["s_L"], kw["s_R"] = cat("s_L2"), cat("s_R2")
    return kw
