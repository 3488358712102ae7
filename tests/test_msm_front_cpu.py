"""The index arithmetic of the MSM's partition front (bazuka_amd/csrc/msm_front.cuh: signed recoding, bin of a key, bin bases, tile offsets, the staged
and the chunked bin pass) on the CPU: tests/host/msm_front_check.hip runs the four passes as plain loops over the functions the kernels call, for
n in {1, 255, 4097, 70 001}, c in {12, 13, 16} and seven scalar mixes, in arrays sized as the call's workspace.  build() compiles it with the address and
undefined-behaviour sanitizers into a program of its own; an out-of-range index aborts it."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_partition_front_model_under_sanitizers():
    exe = os.path.join(HERE, "host", "_msm_front_check")
    assert os.path.exists(exe), "tests/host/_msm_front_check not built (build() compiles it)"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "msm_front_check ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
