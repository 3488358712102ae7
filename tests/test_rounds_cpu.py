"""The staging-round cutter of the batched paths (bazuka_amd/csrc/bzk_rounds.h cut_rounds, round_caps) on the CPU: tests/host/rounds_check.hip
asserts the cutter's rules - the rounds partition the records in order, each holds one, none exceeds the record limit, one exceeds the weight
limit only alone, each is maximal, cap and cap_bytes are the maxima - for n in {0, 1, 2, 3, 4, 5, 8, 9} under limits of 4 records and weight 100
(all zero, an exact fit, just over, one oversized record in three places, a seeded mix), and the two boundaries of the shipped limits (2^16
records, 64 MiB).  build() compiles it with the address and undefined-behaviour sanitizers into a program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_round_cutter_rules_under_sanitizers():
    exe = os.path.join(HERE, "host", "_rounds_check")
    assert os.path.exists(exe), "tests/host/_rounds_check not built (build() compiles it)"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "cases hold" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
