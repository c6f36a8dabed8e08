"""The plan of the mixed verifier queues and the layout of their staging buffer (mpc_bulletproof_amd/csrc/queue_plan.h) on the CPU, under
sanitizers: tests/csrc/queue_plan_host_test.cpp -- a stand-alone program with its own main: crafted queues against recorded plans,
120 000 random queues against the plan's invariants, the layout's rules -- is compiled with the host compiler with
-fsanitize=address,undefined and run.  No GPU, nothing loaded into Python, no preloaded library."""
import os

from test_pool_workers_cpu import INC, ROOT, build_and_run

SRC = os.path.join(ROOT, "tests", "csrc", "queue_plan_host_test.cpp")


def test_the_header_has_no_hip_include():
    txt = open(os.path.join(INC, "queue_plan.h")).read()
    includes = [ln.split()[1] for ln in txt.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_plans_and_staging_layout_under_a_sanitizer(tmp_path):
    build_and_run(tmp_path, "address,undefined", [SRC])
