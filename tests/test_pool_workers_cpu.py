"""The worker set of bpgpu_pool (mpc_bulletproof_amd/csrc/pool_workers.hpp) on the CPU, under sanitizers: tests/csrc/pool_host_test.cpp
-- a stand-alone program with its own main that drives 1, 3 and 32 workers through 1 000 rounds of fake jobs -- is compiled with the
host compiler twice, with -fsanitize=thread and with -fsanitize=address,undefined, and both binaries run.  No GPU, nothing loaded
into Python, no preloaded library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "pool_host_test.cpp")
INC = os.path.join(ROOT, "mpc_bulletproof_amd", "csrc")


def test_the_header_has_no_hip_include():
    txt = open(os.path.join(INC, "pool_workers.hpp")).read()
    includes = [ln.split()[1] for ln in txt.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def build_and_run(tmp_path, sanitizer, sources, extra=()):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pool_test")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all", "-I", INC, *extra, "-o", exe,
           "-x", "c++", *sources]
    # the sanitizer's runtime linked into the program where the compiler has it as an archive (the program then runs the same in any
    # environment), the compiler's default otherwise
    static = ["-static-lib%ssan" % s for s in {"thread": ["t"], "address,undefined": ["a", "ub"]}[sanitizer]]
    if subprocess.call(cmd + static, stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "all passed" in r.stdout and "Sanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("sanitizer", ("thread", "address,undefined"))
def test_rounds_of_fake_jobs_under_a_sanitizer(tmp_path, sanitizer):
    build_and_run(tmp_path, sanitizer, [SRC])


@pytest.mark.parametrize("sanitizer", ("thread", "address,undefined"))
def test_pool_logic_against_fake_contexts_under_a_sanitizer(tmp_path, sanitizer):
    """tests/csrc/pool_api_host_test.cpp: bpgpu_pool.hip itself, compiled as host C++ against fakes of the single-context entry points
    and of its four HIP calls (the HIP headers are needed, no HIP library and no device): shares and pointers per slot, handles per
    distinct device, all-or-nothing creation and options, refusals that wake nobody, a slot failing at run time, the combined check's
    hand-over, the in-place rule for page-locked operands"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    build_and_run(tmp_path, sanitizer, [os.path.join(INC, "bpgpu_pool.hip"), os.path.join(ROOT, "tests", "csrc", "pool_api_host_test.cpp")],
                  extra=["-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include")])
