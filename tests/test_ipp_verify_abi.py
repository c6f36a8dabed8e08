"""The batched InnerProductProof::verify entry points (include/bpgpu.h, bpgpu_ipp_verify_*) on the CPU: exported, bound, declared
for Rust, and every one of them answers a missing operand with BPGPU_E_ARG and a bad (n, k) with BPGPU_E_LEN before anything
touches a device or the context.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bpgpu_ipp_verify_batch", "bpgpu_ipp_verify_batch_dev", "bpgpu_ipp_verify_gens", "bpgpu_ipp_verify_fs"]


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
        assert callable(getattr(m.BpGpu, name[len("bpgpu_"):])), name


def test_header_states_layouts_and_the_factor_length_rule():
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    block = " ".join(hdr[hdr.index("InnerProductProof::verify --"):hdr.index("int bpgpu_ipp_verify_fs")].replace("*", " ").split())
    for phrase in ("nb x k x 64 B (proof-major)", "ab: nb x 2 x 32 B", "creation order", "exactly n entries per proof", ".take(G.len())",
                   "BPGPU_E_LEN", "BPGPU_E_GENS", "bpgpu_input_flag", "ok[p] = 0", "after innerproduct_domain_sep"):
        assert phrase in block, phrase


def _calls(lib, ctx, g, buf, nb, n, k, missing=None):
    """the four entry points with every operand = buf, except the operand named `missing` (None: none missing)"""
    def a(name):
        return None if name == missing else buf
    nb, n, k = C.c_size_t(nb), C.c_size_t(n), C.c_size_t(k)
    return {
        "batch": lib.bpgpu_ipp_verify_batch(ctx, nb, n, k, a("Q"), a("Gf"), a("Hf"), a("G"), a("H"), 1, a("P"), a("L"), a("R"), a("ab"),
                                            a("ch"), a("ok"), None),
        "batch_dev": lib.bpgpu_ipp_verify_batch_dev(ctx, nb, n, k, a("Q"), a("Gf"), a("Hf"), a("G"), a("H"), 1, a("P"), a("L"), a("R"),
                                                    a("ab"), a("ch"), a("ok"), None),
        "gens": lib.bpgpu_ipp_verify_gens(ctx, g, nb, n, k, a("Q"), a("Gf"), a("Hf"), a("P"), a("L"), a("R"), a("ab"), a("ch"), a("ok"),
                                          None),
        "fs": lib.bpgpu_ipp_verify_fs(ctx, None, nb, n, k, a("Q"), a("Gf"), a("Hf"), a("G"), a("H"), 1, a("P"), a("L"), a("R"), a("ab"),
                                      a("ch"), a("ok"), None),
    }


def test_null_context_and_operands_are_rejected_without_a_device():
    m, lib = _lib()
    buf = (C.c_uint8 * 4096)()
    # no context (and, for _gens, no generators)
    assert set(_calls(lib, None, None, buf, 4, 8, 3).values()) == {m.lib.E_ARG}
    assert lib.bpgpu_ipp_verify_gens(buf, None, C.c_size_t(4), C.c_size_t(8), C.c_size_t(3), buf, buf, buf, buf, buf, buf, buf, buf, buf,
                                     None) == m.lib.E_ARG
    # a context that is never looked at (a buffer of zeros stands in for it), one operand missing at a time
    for missing in ("Q", "Gf", "Hf", "P", "L", "R", "ab", "ch", "ok"):
        assert set(_calls(lib, buf, buf, buf, 4, 8, 3, missing).values()) == {m.lib.E_ARG}, missing
    for missing in ("G", "H"):      # (not operands of the resident-generator form)
        r = _calls(lib, buf, buf, buf, 4, 0, 3, missing)   # n = 0 != 2^3: the forms that do not miss an operand stop at the length check
        assert (r["batch"], r["batch_dev"], r["fs"], r["gens"]) == (m.lib.E_ARG,) * 3 + (m.lib.E_LEN,), missing


def test_bad_lengths_are_rejected_without_a_device():
    m, lib = _lib()
    buf = (C.c_uint8 * 4096)()
    for n, k in ((8, 2), (7, 3), (0, 0), (3, 1), (1 << 32, 32), (2, 33)):
        assert set(_calls(lib, buf, buf, buf, 4, n, k).values()) == {m.lib.E_LEN}, (n, k)
    # the length check comes before the empty batch's BPGPU_OK
    assert set(_calls(lib, buf, buf, buf, 0, 8, 2).values()) == {m.lib.E_LEN}
