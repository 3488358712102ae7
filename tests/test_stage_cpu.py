"""The staging loop of the host-pointer batch calls (bazuka_amd/csrc/bzk_stage.h Stage, bzk_rounds.h round_bases) on the CPU: tests/host/stage_check.hip
runs it with memcpy / memset as its device operations on heap blocks of exactly the declared sizes and a host lambda as the kernel, for n in
{0, 1, 2, 3, 4, 5, 8, 9} under limits of 4 records and weight 100 (all zero, an exact fit, just over, one oversized record in three places, a seeded
mix; the boundaries are cut_rounds' own) and three column sets: fixed inputs with an output and an optional output, present and absent; the byte
column with its (m + 1) offsets and a padding of 8; records staged as they stand with round-relative begin / end.  Every output row is what the lambda
makes of that row's inputs, each round runs uploads, lambda, downloads in that order, the registered secrets are zero at return, one synchronise ends
the call; and with each operation of a three-round call failing in turn the call answers BZK_E_DEVICE, runs nothing more but the overwrites and their
synchronise, and leaves the secrets zero.  build() compiles it with the address and undefined-behaviour sanitizers into a program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_staging_loop_under_sanitizers():
    exe = os.path.join(HERE, "host", "_stage_check")
    assert os.path.exists(exe), "tests/host/_stage_check not built (build() compiles it)"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "cases hold" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
