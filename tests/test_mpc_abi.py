"""The two-party prover's entry points (include/bpgpu.h, bpgpu_mpc_*) on the CPU: exported, bound, declared for Rust, and every one of
them returns BPGPU_E_ARG for a missing context, session or operand before anything touches a device.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bpgpu_mpc_prover_commit", "bpgpu_mpc_prover_polys_mask", "bpgpu_mpc_prover_polys_finish", "bpgpu_mpc_prover_ipp_begin",
       "bpgpu_mpc_ipp_mask", "bpgpu_mpc_ipp_round"]


def _lib():
    import mpc_bulletproof_amd as m
    return m, C.CDLL(m.lib.SO_PATH)


def test_entry_points_are_exported_bound_and_declared_for_rust():
    m, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in m.lib.SYMBOLS, name
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert "pub fn %s(" % name in rs, name
    for meth in ("mpc_prover_commit", "mpc_prover_polys_mask", "mpc_prover_polys_finish", "mpc_prover_ipp_begin", "mpc_ipp_mask",
                 "mpc_ipp_round"):
        assert callable(getattr(m.BpGpu, meth)), meth


def test_header_states_the_plane_convention_and_every_layout():
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    block = hdr[hdr.index("two-party prover: ONE party's local arithmetic"):hdr.index("int bpgpu_mpc_prover_commit")]
    for phrase in ("v = s_0 + s_1 + c", "m_0 + m_1 = alpha (s_0 + s_1)", "ark-ff Montgomery form", "canonical little endian",
                   "nb x J x 3 (x, y, z) x 3 x len", "nb x J x 2 (d, e) x 3 x len", "nb x J x 2 (d, e) x len",
                   "nb x 3 x 3 x 64 B", "nb x 3 x 6", "nb x 3 x 5 x 64 B", "2 (padded_n - 1) triples", "6n triples"):
        assert phrase in " ".join(block.replace("*", " ").split()), phrase


def test_null_context_session_and_operands_are_rejected_without_a_device():
    m, lib = _lib()
    E = m.lib.E_ARG
    z, n = C.c_size_t(0), C.c_size_t(4)
    buf = (C.c_uint8 * 4096)()
    h = C.c_void_p()
    assert lib.bpgpu_mpc_prover_commit(None, None, None, n, n, None, None, None, None, None, None, None) == E
    assert lib.bpgpu_mpc_prover_commit(None, buf, C.byref(h), n, n, buf, buf, buf, buf, buf, buf, buf) == E
    assert lib.bpgpu_mpc_prover_polys_mask(None, None, None, None, None, None, None, None) == E
    assert lib.bpgpu_mpc_prover_polys_mask(None, buf, buf, buf, buf, None, buf, buf) == E
    assert lib.bpgpu_mpc_prover_polys_finish(None, None, None, None, None, None, None) == E
    assert lib.bpgpu_mpc_prover_polys_finish(None, buf, buf, buf, buf, buf, buf) == E
    assert lib.bpgpu_mpc_prover_ipp_begin(None, None, None, n, z, None, None, None, None) == E
    assert lib.bpgpu_mpc_prover_ipp_begin(None, buf, buf, n, z, buf, buf, buf, C.byref(h)) == E
    assert lib.bpgpu_mpc_ipp_mask(None, None, None, None) == E
    assert lib.bpgpu_mpc_ipp_mask(None, buf, buf, buf) == E
    assert lib.bpgpu_mpc_ipp_round(None, None, None, None, None) == E
    assert lib.bpgpu_mpc_ipp_round(None, buf, buf, buf, buf) == E
    assert not h.value
