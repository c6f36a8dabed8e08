"""The two-phase prover's entry points (include/bpgpu.h, bpgpu_r1cs_prove_fs2_begin / _finish and their _dev forms) and the wire
verifier with a gadget label (bpgpu_r1cs_verify_batch_wire2 / _dev) on the CPU: exported, bound, declared for Rust with the header's
argument counts, and they answer a missing context with BPGPU_E_ARG and a missing device with BPGPU_E_DEVICE.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of arguments
NEW = {"bpgpu_r1cs_prove_fs2_begin": 18,            # ctx, gens, circuit, nb, n1, states, label, 6 operands, blindings, session, 3 results
       "bpgpu_r1cs_prove_fs2_begin_dev": 18,
       "bpgpu_r1cs_prove_fs2_finish": 17,           # ctx, gens, circuit, session, 8 operands, 5 results
       "bpgpu_r1cs_prove_fs2_finish_dev": 17,
       "bpgpu_r1cs_verify_batch_wire2": 11,         # bpgpu_r1cs_verify_batch_wire's ten and the label
       "bpgpu_r1cs_verify_batch_wire2_dev": 11}


def _lib():
    import mpc_bulletproof_amd as m
    return m, C.CDLL(m.lib.SO_PATH)


def test_entry_points_are_exported_bound_and_declared_with_their_argument_counts():
    m, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert name in m.lib.SYMBOLS, name
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        rdecl = re.search(r"pub fn %s\(([^;]*)\)\s*->" % name, rs, re.S)
        assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == nargs, name
        assert callable(getattr(m.BpGpu, name[len("bpgpu_"):])), name


def test_header_documents_the_calls():
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    block = " ".join(hdr[hdr.index("in TWO calls around the gadget"):hdr.index("int bpgpu_r1cs_prove_fs2_begin(")].replace("*", " ").split())
    for phrase in ("i_blinding1 o_blinding1 s_blinding1", "i_blinding2 o_blinding2 s_blinding2 tb1 tb3 tb4 tb5 tb6", "nb x 3 x 64: A_I1 A_O1 S1",
                   "nb x (11 + 2k) x 64", "t_x t_x_blinding e_blinding a b", "proof_len = 1 + 14 32 + (2k + 2) 32", "version byte 1",
                   "y z u x w u_1..u_k", "e_blinding = x((i1 + u i2) + x((o1 + u o2) + x(s1 + u s2)))", "[1; n1] ++ [u; n2 + pad]",
                   "BPGPU_E_LEN for n1 >= n", "BPGPU_E_GENS", "bpgpu_set_shard(world > 1)", "bpgpu_input_flag", "session != NULL on _begin",
                   "nb == 0: BPGPU_OK with session left NULL", "bpgpu_prover_destroy frees an abandoned one", "without a synchronise"):
        assert phrase in block, phrase
    # the one-call prover keeps refusing parametric circuits, in its own words
    assert "round trip is inherent" in hdr
    wire = " ".join(hdr[hdr.index("bpgpu_r1cs_verify_batch_wire for ONE two-phase circuit"):hdr.index("int bpgpu_r1cs_verify_batch_wire2(")].split())
    assert "version-1 proof" in wire and "gadget" in wire


def test_null_context_is_rejected():
    m, lib = _lib()
    buf = (C.c_uint8 * 4096)()
    sess = C.c_void_p()
    for name in ("bpgpu_r1cs_prove_fs2_begin", "bpgpu_r1cs_prove_fs2_begin_dev"):
        assert getattr(lib, name)(None, buf, buf, C.c_size_t(1), C.c_size_t(0), buf, buf, *([buf] * 7), C.byref(sess), buf, buf, buf) == m.lib.E_ARG, name
        assert getattr(lib, name)(None, None, None, C.c_size_t(0), C.c_size_t(0), *([None] * 13)) == m.lib.E_ARG, name
        assert not sess.value
    for name in ("bpgpu_r1cs_prove_fs2_finish", "bpgpu_r1cs_prove_fs2_finish_dev"):
        assert getattr(lib, name)(None, buf, buf, C.byref(sess), *([buf] * 13)) == m.lib.E_ARG, name
        assert getattr(lib, name)(None, None, None, None, *([None] * 13)) == m.lib.E_ARG, name
    for name in ("bpgpu_r1cs_verify_batch_wire2", "bpgpu_r1cs_verify_batch_wire2_dev"):
        assert getattr(lib, name)(None, buf, buf, C.c_size_t(1), C.c_size_t(0), C.c_size_t(1 + 16 * 32), buf, buf, buf, buf, buf) == m.lib.E_ARG, name


def test_without_a_device_the_calls_answer_e_device():
    """past the shape checks the first thing _begin and the wire verifier do is select the context's device: with none in the machine
    that fails (a zeroed block stands in for the context -- nothing else of it is read before -- and hand-made headers for the
    handles).  _finish needs a session that only _begin makes: without one it answers BPGPU_E_ARG whatever the machine."""
    m, lib = _lib()
    fake_ctx = (C.c_uint8 * (1 << 16))()
    gens = (C.c_size_t * 8)(4)                 # bpgpu_gens: capacity first
    circ = (C.c_size_t * 16)(2, 2, 0, 1, 1)    # bpgpu_circuit: q, n, m, nnz, nchi
    buf = (C.c_uint8 * 4096)()
    sess = C.c_void_p()
    for name in ("bpgpu_r1cs_prove_fs2_finish", "bpgpu_r1cs_prove_fs2_finish_dev"):
        assert getattr(lib, name)(fake_ctx, gens, circ, C.byref(sess), *([buf] * 13)) == m.lib.E_ARG, name
    if lib.bpgpu_device_count() > 0:
        return
    ctx = C.c_void_p()
    assert lib.bpgpu_create(0, C.byref(ctx)) == m.lib.E_DEVICE and not ctx.value
    for name in ("bpgpu_r1cs_prove_fs2_begin", "bpgpu_r1cs_prove_fs2_begin_dev"):
        rc = getattr(lib, name)(fake_ctx, gens, circ, C.c_size_t(1), C.c_size_t(1), buf, buf, buf, buf, buf, buf, buf, None, buf,
                                C.byref(sess), None, None, None)
        assert rc == m.lib.E_DEVICE and not sess.value, name
    for name in ("bpgpu_r1cs_verify_batch_wire2", "bpgpu_r1cs_verify_batch_wire2_dev"):
        rc = getattr(lib, name)(fake_ctx, gens, circ, C.c_size_t(1), C.c_size_t(1), C.c_size_t(1 + 16 * 32 + 2 * 32), buf, buf, buf, buf, buf)
        assert rc == m.lib.E_DEVICE, name
