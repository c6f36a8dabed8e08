"""bpgpu_r1cs_constraints_satisfied / _dev and bpgpu_mpc_constraints_eval (include/bpgpu.h) on the CPU: exported, bound and declared
for Rust with the header's argument counts; their refusals on arguments come back before a device is touched; and a self-check of
the inputs that tests/test_gpu_satisfied.py runs on the GPU: in the model every generated witness satisfies its circuit and every
broken() one does not.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

import circuit_gen as cg
import satisfied_cases as sc

N = sc.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of arguments
NEW = {"bpgpu_r1cs_constraints_satisfied": 12,      # ctx, circuit, nb, 3 planes, v, gadget challenges, ok, 2 indices, residuals
       "bpgpu_r1cs_constraints_satisfied_dev": 12,
       "bpgpu_mpc_constraints_eval": 9}             # ctx, circuit, nb, 3 planes, v, gadget challenges, residuals


def _lib():
    import mpc_bulletproof_amd as m
    return m, C.CDLL(m.lib.SO_PATH)


def test_entry_points_are_exported_bound_and_declared_with_their_argument_counts():
    m, lib = _lib()
    from mpc_bulletproof_amd._abi import PROTOS
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert name in m.lib.SYMBOLS, name
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        rdecl = re.search(r"pub fn %s\(([^;]*)\)\s*->" % name, rs, re.S)
        assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == nargs, name
        assert len(PROTOS[name][1]) == nargs and getattr(m.lib._lib, name).argtypes == PROTOS[name][1], name
        assert callable(getattr(m.BpGpu, name[len("bpgpu_"):])), name


def test_header_documents_the_calls():
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    block = " ".join(hdr[hdr.index("Prover::constraints_satisfied (prover.rs:405-409)"):hdr.index("int bpgpu_r1cs_constraints_satisfied(")]
                     .replace("*", " ").split())
    for phrase in ("the committed VALUES", "first_bad_gate", "a_O crosses the ABI", "nothing per row is stored", "bpgpu_input_flag",
                   "bpgpu_circuit_destroy", "nb == 0: BPGPU_OK", "leaves no pool memory behind", "several contexts"):
        assert phrase in block, phrase
    mpc = " ".join(hdr[hdr.index("bpgpu_mpc_constraints_eval --"):hdr.index("int bpgpu_mpc_constraints_eval(")].replace("*", " ").split())
    for phrase in ("mpc_prover.rs:556-568", "modifier plane only", "nb x 3 x q", "Beaver product", "NOT checked"):
        assert phrase in mpc, phrase


def _calls(lib):
    """the three entry points behind one signature: (ctx, circuit, nb, a_L, a_R, a_O, v, chi, out)"""
    def sat(name):
        return lambda ctx, c, nb, aL, aR, aO, v, chi, out: getattr(lib, name)(ctx, c, C.c_size_t(nb), aL, aR, aO, v, chi, out, None, None, None)
    return {"bpgpu_r1cs_constraints_satisfied": sat("bpgpu_r1cs_constraints_satisfied"),
            "bpgpu_r1cs_constraints_satisfied_dev": sat("bpgpu_r1cs_constraints_satisfied_dev"),
            "bpgpu_mpc_constraints_eval": lambda ctx, c, nb, aL, aR, aO, v, chi, out: lib.bpgpu_mpc_constraints_eval(ctx, c, C.c_size_t(nb), aL, aR, aO,
                                                                                                                    v, chi, out)}


def test_null_pointer_and_gadget_challenge_refusals_come_back_without_a_device():
    """a zeroed block stands in for the context -- nothing of it is read before the refusals -- and hand-made headers for the circuit
    handles (q, n, m, nnz, nchi first)"""
    m, lib = _lib()
    E = m.lib.E_ARG
    fake_ctx = (C.c_uint8 * (1 << 16))()
    numeric = (C.c_size_t * 64)(2, 2, 1, 1, 0)
    param = (C.c_size_t * 64)(2, 2, 1, 1, 1)
    no_vars = (C.c_size_t * 64)(2, 0, 0, 1, 0)
    buf = (C.c_uint8 * 4096)()
    for name, call in _calls(lib).items():
        assert call(None, numeric, 1, buf, buf, buf, buf, None, buf) == E, name                # no context
        assert call(fake_ctx, None, 1, buf, buf, buf, buf, None, buf) == E, name               # no circuit
        for hole in range(4):                                                                  # a_L, a_R, a_O, v
            ops = [buf] * 4
            ops[hole] = None
            assert call(fake_ctx, numeric, 1, *ops, None, buf) == E, (name, hole)
        assert call(fake_ctx, numeric, 1, buf, buf, buf, buf, None, None) == E, name           # ok / residuals
        assert call(fake_ctx, numeric, 1, buf, buf, buf, buf, buf, buf) == E, name             # challenges for a numeric circuit
        assert call(fake_ctx, param, 1, buf, buf, buf, buf, None, buf) == E, name              # none for a parametric one
        assert call(fake_ctx, numeric, 0, buf, buf, buf, buf, buf, buf) == E, name             # ... also with nb == 0
        assert call(fake_ctx, numeric, 0, None, None, None, None, None, None) == 0, name       # nb == 0: nothing to do
        assert call(fake_ctx, param, 0, None, None, None, None, buf, None) == 0, name
        if lib.bpgpu_device_count() == 0:
            # past the refusals the first thing a call does is select the context's device; the planes may be absent when n = m = 0
            assert call(fake_ctx, numeric, 1, buf, buf, buf, buf, None, buf) == m.lib.E_DEVICE, name
            assert call(fake_ctx, no_vars, 1, None, None, None, None, None, buf) == m.lib.E_DEVICE, name


# ---- the inputs of tests/test_gpu_satisfied.py, checked in the model
def test_generated_witnesses_satisfy_their_circuits_and_broken_ones_do_not():
    circuits = [(sc.grid_circuit(q, n, m), ()) for q, nb, n, m in sc.GRID]
    for spec in sc.PARAM:
        circ = cg.Circuit(*spec)
        for chi in ([0] * circ.nchi, [N - 1] * circ.nchi, [1] * circ.nchi, [(7919 * (j + 3)) % N for j in range(circ.nchi)]):
            circuits.append((circ, chi))
    for circ, chi in circuits:
        wit = sc.witness_of(circ)
        assert not any(sc.residuals(circ.rows, wit, chi)), (circ.seed, chi)
        assert sc.first_bad_gate(wit) == -1
        bad = sc.residuals(circ.broken().rows, wit, chi)
        first_const = next(r for r, row in enumerate(circ.rows) if any(var == sc.ONE for var, _ in row))
        assert sc.first_bad(bad) == first_const and sum(1 for e in bad if e) == 1, circ.seed


def test_hand_built_rows_cover_every_length_and_edge():
    T = sc.lane_max()
    rows, wit = sc.length_rows(T)
    lengths = [len(r) for r in rows]
    assert set(sc.row_lengths(T)) <= set(lengths) and {T - 1, T, T + 1} <= set(lengths) and max(lengths) >= 257
    es = sc.residuals(rows, wit)
    q = len(rows)
    assert es[q - 4] == 5 and es[q - 3] == 0 and es[q - 2] == 0 and es[q - 1] == T + 2      # the rows of constants only
    assert es[lengths.index(0)] == 0                                                        # the empty row
    assert es[q - 7] == 257 * (N - 1) * (N - 1) % N                                         # the all-(n - 1) row
    assert es[q - 8] == 257 * -pow(1 << 261, -1, N) % N                                     # the row of the heaviest products
    assert es[q - 6] == 0 and any(es)                                                       # explicit zeros; not a satisfied circuit


def test_chi_fault_is_invisible_at_chi_zero():
    for spec in sc.PARAM:
        circ = cg.Circuit(*spec)
        rows, r = sc.chi_fault(circ)
        wit = sc.witness_of(circ)
        assert not any(sc.residuals(rows, wit, [0] * circ.nchi))
        assert sc.first_bad(sc.residuals(rows, wit, [1] * circ.nchi)) == r


def test_with_constant_breaks_exactly_the_named_rows():
    circ = sc.grid_circuit(255, 1, 0)
    wit = sc.witness_of(circ)
    for bad in ((0,), (254,), (17, 200)):
        es = sc.residuals(sc.with_constant(circ.rows, *bad), wit)
        assert [r for r, e in enumerate(es) if e] == list(bad)
