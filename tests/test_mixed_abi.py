"""The mixed-queue group descriptor (bpgpu_verify_group) is laid out alike in the C header, the ctypes binding and the generated
Rust declarations.  CPU only: the C side is measured by the system compiler."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bpgpu.h")
FIELDS = ["circuit", "nb", "n1", "k", "points", "scalars", "challenges", "gadget_challenges", "rho", "ok"]


def _ctypes_group():
    # the binding's module loads libbpgpu.so on import; the structure itself is plain ctypes, so read it from the source
    src = open(os.path.join(ROOT, "mpc_bulletproof_amd", "lib.py")).read()
    m = re.search(r"class VerifyGroup\(C\.Structure\):.*?_fields_ = (\[.*?\])\n", src, flags=re.S)
    assert m, "lib.py has no VerifyGroup structure"
    import ctypes as C
    ns = {"C": C}
    fields = eval(m.group(1), ns)
    return type("VerifyGroup", (C.Structure,), {"_fields_": fields})


def test_header_declares_the_group_and_the_four_entry_points():
    h = open(HDR).read()
    assert re.search(r"typedef struct bpgpu_verify_group \{.*?\} bpgpu_verify_group;", h, flags=re.S)
    for fn in ("bpgpu_r1cs_verify_mixed_combined", "bpgpu_r1cs_verify_mixed_combined_dev", "bpgpu_r1cs_verify_mixed_screened",
               "bpgpu_r1cs_verify_mixed_screened_dev"):
        assert re.search(fn + r"\s*\(bpgpu_ctx \*ctx, const bpgpu_gens \*g, const bpgpu_verify_group \*groups, size_t ngroups", h), fn


@pytest.mark.skipif(shutil.which("cc") is None, reason="no C compiler on this machine")
def test_ctypes_structure_matches_the_c_compiler(tmp_path):
    c = tmp_path / "probe.c"
    body = "".join(f'  printf("%zu\\n", offsetof(bpgpu_verify_group, {f}));\n' for f in FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bpgpu.h"\nint main(void) {\n'
                 '  printf("%zu\\n", sizeof(bpgpu_verify_group));\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    G = _ctypes_group()
    assert [f[0] for f in G._fields_] == FIELDS
    assert got[0] == __import__("ctypes").sizeof(G)
    assert got[1:] == [getattr(G, f).offset for f in FIELDS]


def test_generated_rust_struct_lists_the_same_fields_in_order():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"]) == 0
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\(Clone, Copy\)\]\s*pub struct bpgpu_verify_group \{(.*?)\}", rs, flags=re.S)
    assert m
    fields = re.findall(r"pub (\w+): ([^,]+),", m.group(1))
    assert [f for f, _ in fields] == FIELDS
    types = dict(fields)
    assert types["circuit"] == "*const bpgpu_circuit"
    assert types["nb"] == types["n1"] == types["k"] == "usize"
    assert types["ok"] == "*mut c_void"
    assert all(types[f] == "*const c_void" for f in ("points", "scalars", "challenges", "gadget_challenges", "rho"))
    for fn in ("mixed_combined", "mixed_combined_dev", "mixed_screened", "mixed_screened_dev"):
        assert re.search(r"pub fn bpgpu_r1cs_verify_" + fn + r"\(ctx: \*mut bpgpu_ctx, g: \*const bpgpu_gens, groups: \*const "
                         r"bpgpu_verify_group, ngroups: usize", rs), fn
