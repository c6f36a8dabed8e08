"""The two-party witness sessions of include/bpgpu.h (bpgpu_mpc_witness_*, bpgpu_witness_gate_levels) on the CPU: exported, bound and
declared for Rust with the header's argument counts; every refusal comes back before a device is touched (hand-made headers stand in
for the handles: their leading fields); bpgpu_witness_gate_levels against the helper's own levels; and a self-check of the model that
tests/test_gpu_mpc_witness.py compares the device with.  No GPU needed."""
import ctypes as C
import os
import re

import mpc_witness_cases as mc
import witness_cases as wc

N = mc.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of arguments
NEW = {"bpgpu_witness_gate_levels": 8, "bpgpu_mpc_witness_begin": 11, "bpgpu_mpc_witness_levels_left": 1, "bpgpu_mpc_witness_level_len": 1,
       "bpgpu_mpc_witness_mask": 4, "bpgpu_mpc_witness_combine": 3, "bpgpu_mpc_witness_finish": 5, "bpgpu_mpc_witness_destroy": 2}


def _lib():
    import mpc_bulletproof_amd as m
    return m, m.lib._lib


def test_entry_points_are_exported_bound_and_declared_with_their_argument_counts():
    m, lib = _lib()
    from mpc_bulletproof_amd._abi import PROTOS
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert name in m.lib.SYMBOLS, name
        decl = re.search(r"\b(?:int|void|size_t) %s\s*\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        rdecl = re.search(r"pub fn %s\(([^;]*)\)\s*(?:->|;)" % name, rs, re.S)
        assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == nargs, name
        assert len(PROTOS[name][1]) == nargs and getattr(lib, name).argtypes == PROTOS[name][1], name
        bound = m.lib if name == "bpgpu_witness_gate_levels" else m.BpGpu
        assert callable(getattr(bound, name[len("bpgpu_"):])), name
    assert "pub struct bpgpu_mpc_witness" in rs
    assert PROTOS["bpgpu_mpc_witness_level_len"][0] is C.c_size_t and PROTOS["bpgpu_mpc_witness_levels_left"][0] is C.c_size_t


def test_header_states_the_layouts_the_rounds_and_the_refusals():
    hdr = " ".join(open(os.path.join(ROOT, "include", "bpgpu.h")).read().replace("*", " ").split())
    block = hdr[hdr.index("two-party witness synthesis: MpcProver::multiply"):hdr.index("int bpgpu_witness_gate_levels(")]
    for phrase in ("now has its own calls", "nb x 3 x n_inputs x 2", "nb x 3 (x, y, z) x 3 x G", "nb x 2 (d, e) x 3 x G", "nb x 2 (d, e) x G",
                   "ascending gate index", "one _mask / _combine pair per level", "BPGPU_WIT_PLAN_LEVELS1", "BPGPU_GATE_BIT",
                   "bpgpu_set_shard(world > 1)", "_mask twice in a row", "_combine without a _mask", "_mask with no level left",
                   "_finish with a level left", "above 2^30", "nb == 0: BPGPU_OK", "leaves no pool memory behind", "kind 22", "UNMEASURED",
                   "profiles/mpc_witness.log"):
        assert phrase in block, phrase


# ---- the refusals: a zeroed block stands in for the context, hand-made headers for the program and the session
def _prog(n, n1, m, nchi, ninp, bits1=0, bits2=0):
    return (C.c_size_t * 64)(n, n1, m, nchi, ninp, bits1 | bits2 << 32)     # ... | BIT gates of phase 1, of phase 2 (two uint32)


def _session(nb, left, length, masked):
    return (C.c_size_t * 64)(nb, left | length << 32, masked)               # nb | levels left, gates of the next (two uint32) | masked


def test_begin_refusals_come_back_without_a_device():
    m, lib = _lib()
    E = m.lib.E_ARG
    fake_ctx = (C.c_uint8 * (1 << 16))()
    buf = (C.c_uint8 * 4096)()
    numeric, param = _prog(2, 1, 1, 0, 1), _prog(2, 1, 1, 1, 0)

    def call(ctx, w, nb, phase, v, inp, chi, aL=None, aR=None, aO=None, out="out"):
        h = C.c_void_p(1)
        rc = lib.bpgpu_mpc_witness_begin(ctx, w, nb, phase, v, inp, chi, aL, aR, aO, C.byref(h) if out == "out" else None)
        assert out != "out" or not h.value                                    # *out is NULL after a refusal, and for nb == 0
        return rc
    assert call(None, numeric, 1, 0, buf, buf, None) == E                     # no context
    assert call(fake_ctx, None, 1, 0, buf, buf, None) == E                    # no program
    assert call(fake_ctx, numeric, 1, 0, buf, buf, None, out=None) == E       # nowhere to put the session
    for phase in (-1, 3):
        assert call(fake_ctx, numeric, 1, phase, buf, buf, None) == E         # a bad phase
        assert call(fake_ctx, numeric, 0, phase, buf, buf, None) == E
    assert call(fake_ctx, numeric, 1, 0, None, buf, None) == E                # v
    assert call(fake_ctx, numeric, 1, 0, buf, None, None) == E                # inputs
    assert call(fake_ctx, numeric, 1, 0, buf, buf, buf) == E                  # challenges for a numeric program
    for phase in (0, 2):
        assert call(fake_ctx, param, 1, phase, buf, None, None, buf, buf, buf) == E      # none for a parametric one's phase 2
    assert call(fake_ctx, param, 1, 1, buf, None, buf) == E                   # ... and given where phase 1 runs alone
    for hole in range(3):                                                     # planes missing for phase 2
        planes = [buf, buf, buf]
        planes[hole] = None
        assert call(fake_ctx, numeric, 1, 2, buf, buf, None, *planes) == E, hole
    # a BIT gate in the evaluated phase; the phase that holds none is accepted
    bit1, bit2 = _prog(2, 1, 1, 0, 0, bits1=1), _prog(2, 1, 1, 0, 0, bits2=1)
    assert call(fake_ctx, bit1, 1, 0, buf, None, None) == E and call(fake_ctx, bit1, 1, 1, buf, None, None) == E
    assert call(fake_ctx, bit2, 1, 0, buf, None, None) == E and call(fake_ctx, bit2, 1, 2, buf, None, None, buf, buf, buf) == E
    assert call(fake_ctx, bit1, 0, 0, None, None, None) == E
    assert call(fake_ctx, bit1, 0, 2, None, None, None) == 0 and call(fake_ctx, bit2, 0, 1, None, None, None) == 0
    # 3 nb n or 3 nb m above 2^30
    assert call(fake_ctx, _prog(1 << 20, 1 << 20, 0, 0, 0), 342, 0, None, None, None) == m.lib.E_LEN
    assert call(fake_ctx, _prog(0, 0, 1 << 20, 0, 0), 342, 0, buf, None, None) == m.lib.E_LEN
    assert call(fake_ctx, _prog(1, 1, 0, 0, 0), (1 << 30) // 3 + 1, 0, None, None, None) == m.lib.E_LEN
    # nb == 0: nothing to do, no session
    assert call(fake_ctx, numeric, 0, 0, None, None, None) == 0
    assert call(fake_ctx, param, 0, 2, None, None, buf) == 0
    if lib.bpgpu_device_count() == 0:                                         # past the refusals a call selects the context's device
        assert call(fake_ctx, numeric, 1, 0, buf, buf, None) == m.lib.E_DEVICE
        assert call(fake_ctx, bit1, 1, 2, buf, None, None, buf, buf, buf) == m.lib.E_DEVICE
        assert call(fake_ctx, bit2, 1, 1, buf, None, None) == m.lib.E_DEVICE
        assert call(fake_ctx, _prog(1 << 20, 1 << 20, 0, 0, 0), 341, 0, None, None, None) == m.lib.E_DEVICE
    # a context after bpgpu_set_shard(world > 1)
    sharded = (C.c_uint8 * (1 << 16))()
    assert lib.bpgpu_set_shard(sharded, 0, 2) == 0
    assert call(sharded, numeric, 1, 0, buf, buf, None) == E
    assert call(sharded, numeric, 0, 0, None, None, None) == E


def test_round_refusals_come_back_without_a_device():
    m, lib = _lib()
    E = m.lib.E_ARG
    fake_ctx = (C.c_uint8 * (1 << 16))()
    buf = (C.c_uint8 * 4096)()
    idle, masked, done = _session(1, 2, 3, 0), _session(1, 2, 3, 1), _session(1, 0, 0, 0)
    assert lib.bpgpu_mpc_witness_levels_left(idle) == 2 and lib.bpgpu_mpc_witness_level_len(idle) == 3
    assert lib.bpgpu_mpc_witness_levels_left(done) == 0 and lib.bpgpu_mpc_witness_level_len(done) == 0
    assert lib.bpgpu_mpc_witness_levels_left(None) == 0 and lib.bpgpu_mpc_witness_level_len(None) == 0
    mask, combine, finish = lib.bpgpu_mpc_witness_mask, lib.bpgpu_mpc_witness_combine, lib.bpgpu_mpc_witness_finish
    for args in ((None, idle, buf, buf), (fake_ctx, None, buf, buf), (fake_ctx, idle, None, buf), (fake_ctx, idle, buf, None)):
        assert mask(*args) == E                                               # null pointers
    assert mask(fake_ctx, masked, buf, buf) == E                              # _mask twice in a row
    assert mask(fake_ctx, done, buf, buf) == E                                # _mask with no level left
    for args in ((None, masked, buf), (fake_ctx, None, buf), (fake_ctx, masked, None)):
        assert combine(*args) == E
    assert combine(fake_ctx, idle, buf) == E and combine(fake_ctx, done, buf) == E       # _combine without a _mask
    for args in ((None, done, buf, buf, buf), (fake_ctx, None, buf, buf, buf)):
        assert finish(*args) == E
    assert finish(fake_ctx, idle, buf, buf, buf) == E and finish(fake_ctx, masked, buf, buf, buf) == E   # _finish with a level left
    lib.bpgpu_mpc_witness_destroy(fake_ctx, None)                             # nothing to free
    lib.bpgpu_mpc_witness_destroy(None, None)
    if lib.bpgpu_device_count() == 0:
        assert mask(fake_ctx, idle, buf, buf) == m.lib.E_DEVICE and combine(fake_ctx, masked, buf) == m.lib.E_DEVICE


# ---- bpgpu_witness_gate_levels against the helper's own levels
def _all_cases():
    return wc.cases() + mc.cases()


def test_gate_levels_equal_the_helpers_on_every_case():
    import mpc_bulletproof_amd as m
    for case in _all_cases():
        prog = case.prog
        got = m.lib.witness_gate_levels(*prog.plan_args())
        assert got == mc.gate_levels(prog), case.name
        plan = m.lib.witness_plan(*prog.plan_args(), 1)
        for ph, (lo, hi) in enumerate(((0, prog.phase1), (prog.phase1, prog.n))):
            assert len(set(got[lo:hi])) == plan["levels%d" % (ph + 1)], (case.name, ph)     # every level below the deepest is inhabited
        assert [len(g) for g in mc.level_lists(prog)] == [got[lo:hi].count(l) for lo, hi in ((0, prog.phase1), (prog.phase1, prog.n))
                                                          for l in range(max(got[lo:hi], default=-1) + 1)], case.name


def test_gate_levels_refusals_are_the_plans():
    import pytest
    import mpc_bulletproof_amd as m
    _, lib = _lib()
    with pytest.raises(m.BpGpuError):
        m.lib.witness_gate_levels(2, 2, 0, [0, 0], [0, 1, 1, 1, 1], [0], [1])          # a forward reference
    with pytest.raises(m.BpGpuError):
        m.lib.witness_gate_levels(2, 3, 0, [0, 0], [0, 0, 0, 0, 0], [], [])            # n1 > n
    assert lib.bpgpu_witness_gate_levels(1, 1, 0, bytes(1), (C.c_uint32 * 3)(), None, None, None) == m.lib.E_ARG    # nowhere to put them
    assert m.lib.witness_gate_levels(0, 0, 0, [], [0], [], []) == []


# ---- the model itself
def test_model_opens_to_the_programs_witness_on_every_case():
    for case in mc.cases():
        for nb in (1, 3):
            mo = mc.model(case, nb)
            assert mo.dealer.bad == [] and mo.dealer.mod_mismatch == [], case.name
            for p in range(nb):
                v, inputs, chi = case.prover(p)
                assert tuple(mo.witness[p]) == tuple(case.prog.evaluate(v, inputs, chi)), (case.name, p)
            assert len(mo.rounds) == sum(case.prog.levels()[:2]), case.name
            lvl, p, s = mo.zero_d
            assert mo.rounds[lvl]["opened_ints"][p][0][s] == 0, case.name              # the triple chosen with x = a_L


def test_gadget_cases_are_the_models_gadgets():
    for case in mc.gadget_cases():
        for p in range(len(case.provers)):
            pv = case.model(p)
            assert (pv.a_L, pv.a_R, pv.a_O) == tuple(case.want(p)), (case.name, p)
            assert all(pv.eval(lc) == 0 for lc in pv.constraints), (case.name, p)
        v, inputs, chi = case.prover(0)
        v2, inputs2 = case.breaker(v, inputs)
        q, nchi, rp, kd, ix, cf = wc.circuit_csr(case)
        coeff = [int.from_bytes(cf[32 * t:32 * t + 32], "little") for t in range(len(kd))]
        planes = tuple(case.prog.evaluate(v2, inputs2, chi)) + (v2,)
        rows = [sum(coeff[t] * (chi[j - 1] if j else 1) * (1 if kd[t] == 4 else planes[kd[t]][ix[t]])
                    for j in range(1 + nchi) for t in range(rp[j * q + r], rp[j * q + r + 1])) % N for r in range(q)]
        assert any(rows), case.name                                                      # the broken statement does not hold


def test_cases_cover_what_they_claim():
    edges = mc.case("mpc_edges").prog
    lengths = {edges.row_len(row) for _, _, left, right in edges.gates for row in (left, right)}
    assert set(mc.ROW_LENGTHS) <= lengths and edges.nchi == 3 and 0 < edges.phase1 < edges.n
    assert {g[0] for g in edges.gates[:edges.phase1]} == {mc.MUL, mc.INPUT} == {g[0] for g in edges.gates[edges.phase1:]}
    assert len(mc.level_lists(edges)[-1]) == 1                                           # a level of one gate
    assert mc.case("mpc_edges_p2").prog.phase1 == 0 and mc.case("mpc_edges_p2").prog.levels()[0] == 0
    assert [len(g) for g in mc.level_lists(mc.case("mpc_wide").prog)] == [300, 5]
    assert [len(g) for g in mc.level_lists(mc.case("range_inputs8").prog)] == [8, 1]
    assert (mc.case("mpc_dag24").prog.n, mc.case("mpc_dag70").prog.n) == (24, 70)
    assert all(g[0] != mc.BIT for c in mc.cases() for g in c.prog.gates)
    assert {g[0] for c in mc.cases() for g in c.prog.gates} == {mc.MUL, mc.INPUT}
    assert sum(mc.case("mpc_dag70").prog.levels()[:2]) > 8                               # back = 6: deep
