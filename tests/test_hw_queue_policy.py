"""The hardware-queue policy of libbpgpu.so's load-time constructor (include/bpgpu.h: bpgpu_hw_queues), case by case.  No device is
needed: the policy runs when the library is loaded, before any HIP call.  Every case is a fresh child process that loads the library
with ctypes and prints what bpgpu_hw_queues reports and what libc's getenv("GPU_MAX_HW_QUEUES") returns afterwards -- the C
environment itself, which is what the HIP runtime will read; os.environ is a snapshot taken at interpreter start and shows neither."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO_PATH = os.path.join(ROOT, "mpc_bulletproof_amd", "libbpgpu.so")

CHILD = r"""
import ctypes, json, sys
libc = ctypes.CDLL(None)
libc.getenv.restype, libc.getenv.argtypes = ctypes.c_char_p, [ctypes.c_char_p]
before = libc.getenv(b"GPU_MAX_HW_QUEUES")
lib = ctypes.CDLL(sys.argv[1])
lib.bpgpu_hw_queues.restype, lib.bpgpu_hw_queues.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
inherited, in_force = ctypes.c_int(12345), ctypes.c_int(12345)
rc = lib.bpgpu_hw_queues(ctypes.byref(inherited), ctypes.byref(in_force))
rc_null = lib.bpgpu_hw_queues(None, None)
after = libc.getenv(b"GPU_MAX_HW_QUEUES")
print(json.dumps({"rc": rc, "rc_null": rc_null, "inherited": inherited.value, "in_force": in_force.value,
                  "before": None if before is None else before.decode(), "after": None if after is None else after.decode(),
                  "own_still_set": libc.getenv(b"BPGPU_HW_QUEUES") is not None}))
"""

UNSET, NOT_A_NUMBER = -1, -2      # bpgpu_hw_queues' codes for a variable that is unset / set to something that is not a number


def load_in_child(inherited, own):
    """-> the child's report; inherited / own: the texts of GPU_MAX_HW_QUEUES / BPGPU_HW_QUEUES in its environment, None = unset"""
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "BPGPU_HW_QUEUES")}
    if inherited is not None:
        env["GPU_MAX_HW_QUEUES"] = inherited
    if own is not None:
        env["BPGPU_HW_QUEUES"] = own
    r = subprocess.run([sys.executable, "-c", CHILD, SO_PATH], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["rc"] == 0 and out["rc_null"] == 0
    assert out["before"] == inherited                                   # the child saw the environment this case set up
    assert out["own_still_set"] == (own is not None)                    # the library's own variable is read, never written
    return out


def code(text):
    return UNSET if text is None else int(text) if text.lstrip("-").isdigit() else NOT_A_NUMBER


# (inherited GPU_MAX_HW_QUEUES, BPGPU_HW_QUEUES, GPU_MAX_HW_QUEUES after the load); None = unset
CASES = [
    (None, None, "24"),           # nobody chose: the requirement
    ("4", None, "24"),            # the runtime's default spelled out by a launcher: cannot be told from "nobody chose"
    ("1", None, "24"),
    ("0", None, "24"),
    ("23", None, "24"),           # just below the requirement
    ("24", None, "24"),           # at the requirement: left alone
    ("25", None, "25"),           # above it: never lowered
    ("32", None, "32"),
    ("40", None, "40"),           # above the cap on what the library exports: still the host's value, untouched
    ("garbage", None, "24"),
    ("", None, "24"),             # set but empty: not a number
    ("4", "0", "4"),              # 0: hands off
    (None, "0", None),            # ... also when that leaves the variable unset
    ("garbage", "0", "garbage"),
    ("32", "0", "32"),
    (None, "8", "8"),             # 1..32: exactly that, over any inherited value
    ("4", "8", "8"),
    ("32", "8", "8"),
    ("garbage", "8", "8"),
    ("4", "1", "1"),
    ("4", "32", "32"),
    (None, "33", "24"),           # outside 0..32: ignored, the default policy holds
    ("4", "33", "24"),
    ("32", "33", "32"),
    (None, "-1", "24"),
    ("4", "-1", "24"),
    ("32", "-1", "32"),
    ("4", "eight", "24"),         # not a number: ignored
    ("4", "8x", "24"),
    ("4", "", "24"),
]


@pytest.mark.parametrize("inherited,own,after", CASES)
def test_queue_policy_at_load(inherited, own, after):
    out = load_in_child(inherited, own)
    assert out["after"] == after, out
    assert out["inherited"] == code(inherited), out
    assert out["in_force"] == code(after), out
    if after is not None and after.isdigit() and after != inherited:
        assert int(after) <= 32, out                                    # whatever the library itself exports is at most 32


def test_python_wrapper_reports_what_the_library_did():
    """lib.hw_queues() in a child started under an inherited 4: (4, 24), while the child's os.environ still says 4"""
    env = {k: v for k, v in os.environ.items() if k != "BPGPU_HW_QUEUES"}
    env["GPU_MAX_HW_QUEUES"] = "4"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", "import os, mpc_bulletproof_amd as m; print(m.lib.hw_queues(), os.environ['GPU_MAX_HW_QUEUES'])"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "(4, 24) 4"
