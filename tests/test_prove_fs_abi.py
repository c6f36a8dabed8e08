"""The one-call prover's entry points (include/bpgpu.h, bpgpu_r1cs_prove_fs / _dev) on the CPU: exported, bound, declared for Rust
with the header's argument counts, and they answer a missing context with BPGPU_E_ARG and a missing device with BPGPU_E_DEVICE.
No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bpgpu_r1cs_prove_fs", "bpgpu_r1cs_prove_fs_dev"]
NARGS = 18     # ctx, gens, circuit, nb, 9 operands, 5 results


def _lib():
    import mpc_bulletproof_amd as m
    return m, C.CDLL(m.lib.SO_PATH)


def test_entry_points_are_exported_bound_and_declared_with_their_argument_counts():
    m, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in m.lib.SYMBOLS, name
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert decl and len(decl.group(1).split(",")) == NARGS, name
        rdecl = re.search(r"pub fn %s\(([^;]*)\)\s*->" % name, rs, re.S)
        assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == NARGS, name
        assert callable(getattr(m.BpGpu, name[len("bpgpu_"):])), name


def test_header_documents_the_call():
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    block = " ".join(hdr[hdr.index("Prover::prove (r1cs/prover.rs:412-727) in ONE call"):hdr.index("int bpgpu_r1cs_prove_fs_dev")].replace("*", " ").split())
    for phrase in ("i_blinding o_blinding s_blinding tb1 tb3 tb4 tb5 tb6", "nb x (11 + 2k) x 64", "t_x t_x_blinding e_blinding a b",
                   "proof_len = 1 + 11 32 + (2k + 2) 32", "y z u x w u_1..u_k", "BPGPU_E_LEN for n == 0", "BPGPU_E_GENS",
                   "bpgpu_set_shard(world > 1)", "bpgpu_input_flag", "round trip is inherent", "nb == 0: BPGPU_OK"):
        assert phrase in block, phrase
    assert "Kind 22" in hdr


def test_null_context_is_rejected():
    m, lib = _lib()
    buf = (C.c_uint8 * 4096)()
    for name in NEW:
        assert getattr(lib, name)(None, buf, buf, C.c_size_t(1), *([buf] * 14)) == m.lib.E_ARG, name
        assert getattr(lib, name)(None, None, None, C.c_size_t(0), *([None] * 14)) == m.lib.E_ARG, name


def test_without_a_device_the_calls_answer_e_device():
    """past the shape checks the first thing either call does is select the context's device: with none in the machine that fails
    (a zeroed block stands in for the context -- nothing else of it is read before -- and hand-made headers for the handles)"""
    m, lib = _lib()
    if lib.bpgpu_device_count() > 0:
        return
    ctx = C.c_void_p()
    assert lib.bpgpu_create(0, C.byref(ctx)) == m.lib.E_DEVICE and not ctx.value
    fake_ctx = (C.c_uint8 * (1 << 16))()
    gens = (C.c_size_t * 8)(4)                 # bpgpu_gens: capacity first
    circ = (C.c_size_t * 16)(1, 2, 0, 1, 0)    # bpgpu_circuit: q, n, m, nnz, nchi
    buf = (C.c_uint8 * 4096)()
    for name in NEW:
        rc = getattr(lib, name)(fake_ctx, gens, circ, C.c_size_t(1), buf, buf, buf, buf, buf, buf, None, None, buf, buf, buf, None, None, None)
        assert rc == m.lib.E_DEVICE, name
