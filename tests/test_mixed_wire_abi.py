"""The wire-format mixed-queue descriptor (bpgpu_wire_group) and its four entry points are laid out alike in the C header, the ctypes
binding and the generated Rust declarations, exported by the library, and refuse a missing context or an over-long group list before
anything touches a device.  CPU only: the C side is measured by the system compiler."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bpgpu.h")
FIELDS = ["circuit", "nb", "n1", "proof_len", "proofs", "commitments", "init_states", "gadget_label", "rho", "ok"]
ENTRY_POINTS = ["bpgpu_r1cs_verify_mixed_wire_screened", "bpgpu_r1cs_verify_mixed_wire_screened_dev",
                "bpgpu_r1cs_verify_mixed_wire_combined", "bpgpu_r1cs_verify_mixed_wire_combined_dev"]


def _ctypes_group():
    # the binding's module loads libbpgpu.so on import; the structure itself is plain ctypes, so read it from the source
    src = open(os.path.join(ROOT, "mpc_bulletproof_amd", "lib.py")).read()
    m = re.search(r"class WireGroup\(C\.Structure\):.*?_fields_ = (\[.*?\])\n", src, flags=re.S)
    assert m, "lib.py has no WireGroup structure"
    return type("WireGroup", (C.Structure,), {"_fields_": eval(m.group(1), {"C": C})})


def test_header_declares_the_group_and_the_four_entry_points():
    h = open(HDR).read()
    assert re.search(r"typedef struct bpgpu_wire_group \{.*?\} bpgpu_wire_group;", h, flags=re.S)
    for fn in ENTRY_POINTS:
        assert re.search(fn + r"\s*\(bpgpu_ctx \*ctx, const bpgpu_gens \*g, const bpgpu_wire_group \*groups, size_t ngroups", h), fn
    # the existing descriptor is untouched and comes first
    assert h.index("} bpgpu_verify_group;") < h.index("typedef struct bpgpu_wire_group")


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler on this machine")
def test_ctypes_structure_matches_the_c_compiler(tmp_path):
    c = tmp_path / "probe.c"
    body = "".join(f'  printf("%zu\\n", offsetof(bpgpu_wire_group, {f}));\n' for f in FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bpgpu.h"\nint main(void) {\n'
                 '  printf("%zu\\n", sizeof(bpgpu_wire_group));\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    G = _ctypes_group()
    assert [f[0] for f in G._fields_] == FIELDS
    assert got[0] == C.sizeof(G)
    assert got[1:] == [getattr(G, f).offset for f in FIELDS]


def test_generated_rust_struct_lists_the_same_fields_in_order():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"]) == 0
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\(Clone, Copy\)\]\s*pub struct bpgpu_wire_group \{(.*?)\}", rs, flags=re.S)
    assert m
    fields = re.findall(r"pub (\w+): ([^,]+),", m.group(1))
    assert [f for f, _ in fields] == FIELDS
    types = dict(fields)
    assert types["circuit"] == "*const bpgpu_circuit"
    assert types["nb"] == types["n1"] == types["proof_len"] == "usize"
    assert types["gadget_label"] == "*const u8"
    assert types["ok"] == "*mut c_void"
    assert all(types[f] == "*const c_void" for f in ("proofs", "commitments", "init_states", "rho"))
    for fn in ENTRY_POINTS:
        assert re.search(r"pub fn " + fn + r"\(ctx: \*mut bpgpu_ctx, g: \*const bpgpu_gens, groups: \*const bpgpu_wire_group, ngroups: usize", rs), fn


def test_symbols_are_exported_and_bound():
    import mpc_bulletproof_amd as m
    lib = C.CDLL(m.lib.SO_PATH)
    for fn in ENTRY_POINTS:
        assert hasattr(lib, fn), fn
        assert fn in m.lib.SYMBOLS and len(m.lib.PROTOS[fn][1]) == 5, fn
        assert hasattr(m.BpGpu, fn[len("bpgpu_"):]), fn
    assert C.sizeof(m.lib.WireGroup) == C.sizeof(_ctypes_group())


def test_null_context_and_long_group_lists_are_refused_without_a_device():
    import mpc_bulletproof_amd as m
    lib = m.lib._lib
    E = m.lib.E_ARG
    groups = (m.lib.WireGroup * (m.lib.MIXED_MAX_GROUPS + 1))()
    nf, out = C.c_size_t(7), (C.c_uint8 * 64)(*([7] * 64))
    # stand-ins for the two handles: the list length is checked before either is looked at
    fake_ctx, fake_gens = (C.c_uint8 * 4096)(), (C.c_uint8 * 256)()
    for ctx, g, n in ((None, None, 0), (None, fake_gens, 1), (fake_ctx, fake_gens, m.lib.MIXED_MAX_GROUPS + 1), (fake_ctx, None, 1)):
        assert lib.bpgpu_r1cs_verify_mixed_wire_screened(ctx, g, groups, n, C.byref(nf)) == E
        assert lib.bpgpu_r1cs_verify_mixed_wire_screened_dev(ctx, g, groups, n, C.byref(nf)) == E
        assert lib.bpgpu_r1cs_verify_mixed_wire_combined(ctx, g, groups, n, out) == E
        assert lib.bpgpu_r1cs_verify_mixed_wire_combined_dev(ctx, g, groups, n, out) == E
    assert lib.bpgpu_r1cs_verify_mixed_wire_combined(fake_ctx, fake_gens, groups, 0, None) == E
    assert bytes(out) == bytes([7] * 64)
