"""Inputs and expected outputs of bpgpu_r1cs_prove_fs from the Python model: pm.Prover.prove on a generated circuit
(tests/circuit_gen.py), driven by a replay RNG that hands the model the blindings the GPU call gets.  No GPU needed."""
import random

import circuit_gen as cg
import mpc_dealer as md
import oracle_lib as o

pm = cg.pm
N = pm.N
le, mont = md.le, md.mont


class Replay:
    """the model's RNG interface over a prepared list of scalars"""

    def __init__(self, values):
        self.values = list(values)

    def scalar(self):
        return self.values.pop(0)


def lg_padded(n):
    return max(n - 1, 0).bit_length()


def label(p):
    return cg.LABEL + b" #%d" % p


def model_proof(circ, mgens, p, vkeys, seed):
    """proof p of a batch: the circuit's witness under its own transcript label and blindings -> a record with the call's operands
    for this proof (ark form where the ABI takes it), the model's proof and the expected output bytes"""
    rnd = random.Random(seed * 1000 + p * 2 + int(vkeys))
    n, m = circ.n, circ.m
    vb = [rnd.randrange(N) for _ in range(m)]
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(label(p)))
    info = circ.install(pv, rng=Replay(vb))
    state_in = pv.transcript.state
    bl = [rnd.randrange(N) for _ in range(3)]
    key = bytes(rnd.getrandbits(8) for _ in range(32))
    if vkeys:
        sL = [int.from_bytes(b, "little") for b in md.cut(o.blind_vector(key, 0, n), 32)]
        sR = [int.from_bytes(b, "little") for b in md.cut(o.blind_vector(key, 1, n), 32)]
    else:
        sL, sR = [rnd.randrange(N) for _ in range(n)], [rnd.randrange(N) for _ in range(n)]
    tb = [rnd.randrange(N) for _ in range(5)]
    trace = {}
    rng = Replay(bl + sL + sR + tb)
    proof = pv.prove(mgens, rng, trace=trace)
    assert not rng.values
    order = ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6")
    points = b"".join(pm.p2b(proof[k]) for k in order) + b"".join(map(pm.p2b, proof["L_vec"])) + b"".join(map(pm.p2b, proof["R_vec"]))
    scalars = b"".join(le(proof[k]) for k in ("t_x", "t_x_blinding", "e_blinding", "a", "b"))
    ch = b"".join(le(trace[k]) for k in "yzuxw") + b"".join(le(u) for u, _ in trace["ipp"])
    return dict(
        state_in=state_in, a_L=b"".join(map(mont, circ.a_L[:n])), a_R=b"".join(map(mont, circ.a_R[:n])),
        a_O=b"".join(mont(circ.a_L[i] * circ.a_R[i]) for i in range(n)), s_L=b"".join(map(mont, sL)), s_R=b"".join(map(mont, sR)), key=key,
        v_blinding=b"".join(map(mont, vb)), blindings=b"".join(map(mont, bl + tb)), vb=vb,
        proof=proof, V=info["V"], trace=trace, points=points, scalars=scalars, challenges=ch, state_out=pv.transcript.state,
        wire=pm.r1cs_proof_to_bytes(proof))


def operands(recs, vkeys):
    """the keyword operands of BpGpu.r1cs_prove_fs for a batch of records"""
    cat = lambda k: b"".join(r[k] for r in recs)      # noqa: E731
    kw = dict(states=cat("state_in"), a_L=cat("a_L"), a_R=cat("a_R"), a_O=cat("a_O"), blindings=cat("blindings"),
              v_blinding=cat("v_blinding") or None)
    if vkeys:
        kw["vector_keys"] = cat("key")
    else:
        kw["s_L"], kw["s_R"] = cat("s_L"), cat("s_R")
    return kw
