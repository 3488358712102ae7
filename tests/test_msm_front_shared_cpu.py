"""The index arithmetic of the partition front's shared form (bazuka_amd/csrc/msm_front.cuh FrontPlan::shared: the levels of a full window table feed ONE
bucket set, a bin is the key's high bits, 64-bit intermediate pairs) on the CPU: tests/host/msm_front_shared_check.hip runs the four passes as plain loops over
the functions the kernels call, for n in {1, 63, 4097, 20 011}, c in {11, 16, 19, 20} and eight scalar mixes - whole calls, a prefix of a larger set, a range
of levels, a forced tiny bin capacity, and one bucket that holds a whole vector - in arrays sized as the call's workspace.  build() compiles it with the address
and undefined-behaviour sanitizers into a program of its own; an out-of-range index aborts it."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_shared_partition_front_model_under_sanitizers():
    exe = os.path.join(HERE, "host", "_msm_front_shared_check")
    assert os.path.exists(exe), "tests/host/_msm_front_shared_check not built (build() compiles it)"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "msm_front_shared_check ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
