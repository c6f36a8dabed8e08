"""The entry points that commit the provers' values (include/bpgpu.h, bpgpu_r1cs_commit_values / _dev, bpgpu_mpc_commit_values) on the
CPU: exported, bound, declared for Rust with the header's argument counts, documented, and they answer what needs no device -- a
missing context, the refusals on shapes and pointers, the empty batch -- and a missing device with BPGPU_E_DEVICE.  And the
expectations of tests/commit_cases.py agree with the model prover's own commit().  No GPU needed."""
import ctypes as C
import os
import re

import pytest

import circuit_gen as cg
import commit_cases as cc
import prove_fs_cases as pc

pm = cg.pm
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"bpgpu_r1cs_commit_values": 10, "bpgpu_r1cs_commit_values_dev": 10, "bpgpu_mpc_commit_values": 7}


def _lib():
    import mpc_bulletproof_amd as m
    return m, C.CDLL(m.lib.SO_PATH)


def _fake():
    """a zeroed block for the context (only its mutex and shard fields are read before the device is selected) and a hand-made
    header for the generators (capacity first)"""
    return (C.c_uint8 * (1 << 16))(), (C.c_size_t * 8)(4), (C.c_uint8 * 4096)()


def sz(x):
    return C.c_size_t(x)


def test_entry_points_are_exported_bound_and_declared_with_their_argument_counts():
    m, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    for name, nargs in NARGS.items():
        assert hasattr(lib, name), name
        assert name in m.lib.SYMBOLS, name
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        rdecl = re.search(r"pub fn %s\(([^;]*)\)\s*->" % name, rs, re.S)
        assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == nargs, name
        assert callable(getattr(m.BpGpu, name[len("bpgpu_"):])), name


def test_header_documents_the_calls():
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    block = " ".join(hdr[hdr.index("Prover::commit (r1cs/prover.rs:319-329)"):hdr.index("int bpgpu_r1cs_commit_values_dev")].replace("*", " ").split())
    for phrase in ("ark-ff Montgomery form",                                        # the ark form
                   "the _fs / _wire verifiers take as init_states",                 # the shared init_states convention
                   "64 zero bytes, compressed as 00..00 40", "absorbed as 64 zero bytes",     # the identity encoding
                   "m == 0 is legal", "states_out is the state after the separator",
                   "states_in and states_out go together",
                   "The chain of ONE prover is serial", "32 768 commitments", "9-13 ms", "not measured", "states_in = states_out = NULL",
                   "null context or gens", "null v or v_blinding while nb m > 0", "exactly one of states_in / states_out",
                   "no output at all", "bpgpu_set_shard(world > 1)", "BPGPU_E_LEN for nb m above 2^30", "nb == 0: BPGPU_OK",
                   "BPGPU_E_ARG in the host form", "bpgpu_input_flag", "leaves no pool memory behind", "kind 16", "kind 22",
                   "bpgpu_r1cs_constraints_satisfied takes as v", "bpgpu_r1cs_prove_fs as v_blinding"):
        assert phrase in block, phrase
    mpc = " ".join(hdr[hdr.index("bpgpu_mpc_commit_values -- one party's local half"):hdr.index("int bpgpu_mpc_commit_values")].replace("*", " ").split())
    for phrase in ("mpc_prover.rs:402-456", "nb x 3 x m", "no step needs the party index", "no transcript", "OPENED values", "3 nb m above 2^30"):
        assert phrase in mpc, phrase
    assert re.search(r"#define BPGPU_PROF_KINDS 24\b", hdr)


def test_null_context_is_rejected():
    m, lib = _lib()
    buf = (C.c_uint8 * 4096)()
    for name in ("bpgpu_r1cs_commit_values", "bpgpu_r1cs_commit_values_dev"):
        assert getattr(lib, name)(None, buf, sz(1), sz(1), buf, buf, buf, buf, buf, buf) == m.lib.E_ARG, name
        assert getattr(lib, name)(None, None, sz(0), sz(0), *([None] * 6)) == m.lib.E_ARG, name
        assert getattr(lib, name)(buf, None, sz(1), sz(1), buf, buf, buf, buf, buf, buf) == m.lib.E_ARG, name     # no generators
    assert lib.bpgpu_mpc_commit_values(None, buf, sz(1), sz(1), buf, buf, buf) == m.lib.E_ARG
    assert lib.bpgpu_mpc_commit_values(buf, None, sz(1), sz(1), buf, buf, buf) == m.lib.E_ARG


def test_refusals_that_need_no_device():
    """every one of them is answered before the context's device is selected: a zeroed block stands in for the context"""
    m, lib = _lib()
    E = m.lib
    ctx, gens, b = _fake()
    for name in ("bpgpu_r1cs_commit_values", "bpgpu_r1cs_commit_values_dev"):
        f = getattr(lib, name)
        assert f(ctx, gens, sz(2), sz(3), None, b, b, b, b, b) == E.E_ARG, name               # no v
        assert f(ctx, gens, sz(2), sz(3), b, None, b, b, b, b) == E.E_ARG, name               # no v_blinding
        assert f(ctx, gens, sz(2), sz(3), b, b, b, b, b, None) == E.E_ARG, name               # states_in alone
        assert f(ctx, gens, sz(2), sz(3), b, b, None, b, b, b) == E.E_ARG, name               # states_out alone
        assert f(ctx, gens, sz(2), sz(0), None, None, b, None, None, None) == E.E_ARG, name   # states_in alone, m == 0
        assert f(ctx, gens, sz(2), sz(3), b, b, None, None, None, None) == E.E_ARG, name      # no output
        assert f(ctx, gens, sz(1 << 20), sz((1 << 10) + 1), b, b, b, b, b, b) == E.E_LEN, name      # nb m = 2^30 + 2^20
        assert f(ctx, gens, sz(1 << 40), sz(1 << 40), b, b, b, b, b, b) == E.E_LEN, name            # nb m wraps around 2^64
        assert f(ctx, gens, sz((1 << 30) + 1), sz(0), None, None, b, None, None, b) == E.E_LEN, name
        assert f(ctx, gens, sz(0), sz(3), None, None, b, b, b, b) == 0, name                  # nb == 0
        assert lib.bpgpu_set_shard(ctx, sz(1), sz(2)) == 0
        try:
            assert f(ctx, gens, sz(2), sz(3), b, b, b, b, b, b) == E.E_ARG, name              # a sharded context
        finally:
            assert lib.bpgpu_set_shard(ctx, sz(0), sz(1)) == 0
    f = lib.bpgpu_mpc_commit_values
    assert f(ctx, gens, sz(2), sz(3), None, b, b) == E.E_ARG
    assert f(ctx, gens, sz(2), sz(3), b, None, b) == E.E_ARG
    assert f(ctx, gens, sz(2), sz(3), b, b, None) == E.E_ARG                                  # no output
    assert f(ctx, gens, sz(1 << 19), sz(1 << 10), b, b, b) == E.E_LEN                         # 3 nb m = 3 2^29
    assert f(ctx, gens, sz(0), sz(3), None, None, b) == 0
    assert lib.bpgpu_set_shard(ctx, sz(1), sz(2)) == 0
    try:
        assert f(ctx, gens, sz(2), sz(3), b, b, b) == E.E_ARG
    finally:
        assert lib.bpgpu_set_shard(ctx, sz(0), sz(1)) == 0


def test_the_empty_batch_touches_no_output():
    m, lib = _lib()
    ctx, gens, b = _fake()
    outs = [(C.c_uint8 * 256)(*([0xA5] * 256)) for _ in range(3)]
    for name in ("bpgpu_r1cs_commit_values", "bpgpu_r1cs_commit_values_dev"):
        assert getattr(lib, name)(ctx, gens, sz(0), sz(4), b, b, b, *outs) == 0, name
    assert lib.bpgpu_mpc_commit_values(ctx, gens, sz(0), sz(4), b, b, outs[0]) == 0
    assert all(bytes(x) == b"\xA5" * 256 for x in outs)


def test_without_a_device_the_calls_answer_e_device():
    """past the refusals the first thing a call does is select the context's device: with none in the machine that fails"""
    m, lib = _lib()
    if lib.bpgpu_device_count() > 0:
        return
    ctx, gens, b = _fake()
    for name in ("bpgpu_r1cs_commit_values", "bpgpu_r1cs_commit_values_dev"):
        f = getattr(lib, name)
        assert f(ctx, gens, sz(2), sz(3), b, b, b, b, b, b) == m.lib.E_DEVICE, name
        assert f(ctx, gens, sz(2), sz(3), b, b, None, None, b, None) == m.lib.E_DEVICE, name      # one output, no transcript
        assert f(ctx, gens, sz(2), sz(0), None, None, b, None, None, b) == m.lib.E_DEVICE, name   # m == 0: the chain alone
        assert f(ctx, gens, sz(1 << 20), sz(1 << 10), b, b, b, b, b, b) == m.lib.E_DEVICE, name   # nb m = 2^30: the largest shape
    assert lib.bpgpu_mpc_commit_values(ctx, gens, sz(2), sz(3), b, b, b) == m.lib.E_DEVICE


# ---- the expectations of tests/commit_cases.py against the model prover
@pytest.mark.parametrize("n,m,q", ((2, 0, 3), (3, 2, 7), (5, 5, 12)))
def test_expectations_agree_with_the_model_provers_commit(n, m, q):
    """V and the transcript state of pm.Prover after its commit() calls, for a generated circuit and two provers of it"""
    circ = cg.Circuit(500 + 10 * n + m, n, 0, m, q, 0, "sparse")
    nb = 2
    v = [list(circ.v) for _ in range(nb)]
    _, vb = cc.values(40 + m, nb, m)
    init = [pm.Transcript(pc.label(p)).state for p in range(nb)]
    want = cc.expect(v, vb, pm.G, pm.G, init)
    states = b""
    for p in range(nb):
        pv = pm.Prover(pm.PedersenGens(), pm.Transcript(pc.label(p)))
        info = circ.install(pv, rng=pc.Replay(vb[p]))
        assert info["V"] == want["points"][p], p
        assert [x % pm.N for x in pv.v] == [x % pm.N for x in v[p]] and pv.v_blinding == vb[p]
        states += pv.transcript.state
    assert states == want["states_out"]
    assert len(want["V"]) == 64 * nb * m and len(want["V_compressed"]) == 32 * nb * m
    assert want["V"] == b"".join(pm.p2b(pt) for row in want["points"] for pt in row)


def test_identity_commitments_are_expected_as_zero_bytes():
    """(0, 0) and (x, n - x) over equal bases: 64 zero bytes, 00..00 40, and a chain that absorbed zeros -- over different bases the
    second pair is a point"""
    init = cc.init_states(1)
    v, vb = [[a for a, _ in cc.IDENTITY_PAIRS]], [[b for _, b in cc.IDENTITY_PAIRS]]
    e = cc.expect(v, vb, pm.G, pm.G, init)
    assert e["V"] == bytes(128) and e["V_compressed"] == (bytes(31) + b"\x40") * 2
    tr = pm.Transcript(b"")
    tr.state = init[0]
    tr.r1cs_domain_sep()
    for _ in range(2):
        tr.append_message(b"V", bytes(64))
    assert e["states_out"] == tr.state
    other = cc.expect(v, vb, pm.G, cc.base_H0(), init)
    assert other["V"][:64] == bytes(64) and other["V"][64:] != bytes(64)


def test_edge_batches_hold_every_pair_in_every_route():
    for nb, m in cc.EDGE_SHAPES:
        seen = set()
        for v, vb in cc.edge_batches(8, nb, m):
            assert len(v) == len(vb) == nb and all(len(r) == m for r in v + vb)
            seen |= {(a, b) for rv, rb in zip(v, vb) for a, b in zip(rv, rb)}
        assert set(cc.LISTED_PAIRS) | set(cc.window_pairs(8)) <= seen, (nb, m)
    import window_digits as wd
    half = 1 << 7
    for s, t in cc.window_pairs(8):
        for x in (s, t):
            assert all(d in (-half, half - 1) for d in wd.digits(x, 8)[:-1])
