"""The index arithmetic of the passes a table call's partition front runs (bazuka_amd/csrc/msm_front.cuh FrontPlan::table_stage / table_widen / table_cell:
the scatter pass stages tile-local 32-bit words, four levels a round, and widens them to 64-bit pairs that carry their level; the bin pass ranks by (bucket,
level) cells with no barrier between strides) on the CPU: tests/host/msm_front_table_check.hip runs the four passes as plain loops over the functions the
kernels call, for every window size c in 11 .. 20, n in {1, 63, 4097, 20 011} and eight scalar mixes - whole calls, a prefix of a larger set, levels [3, 8),
and one bucket that holds a whole vector - in arrays sized as the kernels' LDS arrays and the call's workspace, the second sweep of the bin pass walked
backwards.  Beside the properties of the shared check it asserts that the levels inside every bucket are non-decreasing, that no cell index leaves the
counters for any c, and that the plan refuses the shapes whose cells or levels do not fit.  build() compiles it with the address and undefined-behaviour
sanitizers into a program of its own; an out-of-range index aborts it."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_table_front_model_under_sanitizers():
    exe = os.path.join(HERE, "host", "_msm_front_table_check")
    assert os.path.exists(exe), "tests/host/_msm_front_table_check not built (build() compiles it)"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "msm_front_table_check ok: 991 cases" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
