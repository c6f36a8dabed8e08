"""Operands of bpgpu_r1cs_prove_values for the gadget cases of tests/witness_cases.py, and the chain of existing host-form calls that
the one call replaces: the yardstick of tests/test_gpu_prove_values.py and tests/test_gpu_pool_prove_values.py.  The per-prover
operands are drawn the way tests/test_gpu_prove_fs2_onecall.py: record draws them (own transcript label, seeded blindings and keys),
without the Python model's proof.  No GPU needed to import."""
import random

import witness_cases as wc
from prove_fs_cases import label, lg_padded

pm = wc.pm
N = wc.N
mont = wc.mont
CAP = 16
LABEL = wc.SHUFFLE_LABEL
ONE_PHASE = ("range8x2", "example")
TWO_PHASE = ("shuffle2", "shuffle4", "composite")
FIELDS = ("ok", "first_bad_row", "first_bad_gate", "V", "V_compressed", "points", "scalars", "wire", "challenges", "states", "chi", "planes")

_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = wc.range_case(8, 2) if name == "range8x2" else wc.case(name)
    return _cases[name]


def two_phase(name):
    return case(name).prog.nchi == 1


def proof_len(name):
    return 1 + (14 if two_phase(name) else 11) * 32 + (2 * lg_padded(case(name).prog.n) + 2) * 32


def row_bytes(name):
    """bytes per prover of every per-prover output"""
    prog = case(name).prog
    k = lg_padded(prog.n)
    return dict(V=64 * prog.m, V_compressed=32 * prog.m, points=64 * (11 + 2 * k), scalars=160, wire=proof_len(name), challenges=32 * (5 + k),
                states=32, chi=32, a_L=32 * prog.n, a_R=32 * prog.n, a_O=32 * prog.n, ok=4, first_bad_row=8, first_bad_gate=8)


_circuits = {}


def circuit_csr(name):
    if name not in _circuits:
        _circuits[name] = wc.circuit_csr(case(name))
    return _circuits[name]


def handles(maker, name):
    """(circuit, program) of a case on a BpGpu or a BpPool"""
    c = case(name)
    q, nchi, rp, kd, ix, cf = circuit_csr(name)
    assert nchi == c.prog.nchi
    circ = maker.circuit_create_param(q, 1, rp, kd, ix, cf, c.prog.n, c.prog.m) if nchi else maker.circuit_create(rp, kd, ix, cf, c.prog.n, c.prog.m)
    return circ, maker.witness_create(*c.prog.create_args())


def ark(values):
    return b"".join(map(mont, values))


def operands(name, nb, keys, bad=None):
    """the keyword operands of BpGpu.r1cs_prove_values for nb provers; prover `bad` (if any) with the case's breaker applied to its
    values: a statement that does not hold.  Every other prover's operands do not depend on nb, keys' alternative or bad."""
    c = case(name)
    prog = c.prog
    two = two_phase(name)
    init, v, inputs, vb, bl, ks, sL, sR = ([] for _ in range(8))
    for p in range(nb):
        pv, pin, _ = c.prover(p % len(c.provers))
        if p == bad:
            pv, pin = c.breaker(pv, pin)
        rnd = random.Random(7000 + 10 * p + 1000 * (ONE_PHASE + TWO_PHASE).index(name))
        init.append(pm.Transcript(label(p)).state)
        v.append(ark(x % N for x in pv))
        inputs.append(ark(x for pair in pin for x in pair))
        vb.append(ark(rnd.randrange(N) for _ in range(prog.m)))
        bl.append(ark(rnd.randrange(N) for _ in range(11 if two else 8)))
        ks.append(bytes(rnd.getrandbits(8) for _ in range(64 if two else 32)))
        sL.append(ark(rnd.randrange(N) for _ in range(prog.n)))
        sR.append(ark(rnd.randrange(N) for _ in range(prog.n)))
    cat = b"".join
    kw = dict(init_states=cat(init), v=cat(v), v_blinding=cat(vb), inputs=cat(inputs) or None, blindings=cat(bl),
              gadget_label=LABEL if two else None)
    if keys:
        kw["vector_keys"] = cat(ks)
    else:
        kw["s_L"], kw["s_R"] = cat(sL), cat(sR)
    return kw


def chain(gpu, gens, circ, w, name, nb, ops):
    """the chain of existing host-form calls on the operands of the one call -> the twelve outputs, in ProveValues' order"""
    prog = case(name).prog
    n, m, q = prog.n, prog.m, circuit_csr(name)[0]
    src = {key: ops[key] for key in ("s_L", "s_R", "vector_keys") if key in ops}
    V, Vc, st = gpu.r1cs_commit_values(gens, nb, m, ops["v"], ops["v_blinding"], states=ops["init_states"])
    if not two_phase(name):
        planes = gpu.r1cs_witness_synthesize(w, nb, n, 0, v=ops["v"], inputs=ops["inputs"])
        ok, row, gate, _ = gpu.r1cs_constraints_satisfied(circ, nb, q, *planes, v=ops["v"])
        pts, sc, wire, ch, so = gpu.r1cs_prove_fs(gens, circ, nb, n, m, st, *planes, ops["blindings"], v_blinding=ops["v_blinding"], **src)
        chi = None
    else:
        pts, sc, wire, ch, so, chi, planes = gpu.r1cs_prove_fs2(gens, circ, w, nb, n, m, st, LABEL, ops["blindings"], v=ops["v"],
                                                                inputs=ops["inputs"], v_blinding=ops["v_blinding"], want_witness=True, **src)
        ok, row, gate, _ = gpu.r1cs_constraints_satisfied(circ, nb, q, *planes, v=ops["v"], gadget_challenges=chi)
    return ok, row, gate, V, Vc, pts, sc, wire, ch, so, chi, planes


def rows(name, field, data, which):
    """the rows of the provers `which` of one per-prover output"""
    per = row_bytes(name)["a_L" if field == "planes" else field]
    return b"".join(data[per * p:per * (p + 1)] for p in which)
