"""The NTT passes replayed on the CPU with their bound arguments asserted (tests/host/_ntt_pass_check, built by build() with BZK_FP28_CHECK and the host
sanitizers): whole transforms through the plan's passes - the lone stage, the radix-4 rounds, the three first-load modes, the inter-pass and the final
store - on the value patterns of tests/fr_value_cases.py plus uniform random values.  The program aborts where ka * kb > 70 at a product, a sub3 limb
could underflow or a word wrap, a value given to repack_to32 reaches 2^256, or k > 35 at from29_scaled; what it writes is compared here with the oracle
(co.ntt, co.groth16_h), never with the library."""
import os
import re
import subprocess

import pytest

import fr_value_cases as V
from fr_value_cases import raw_fr_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "host", "_ntt_pass_check")
MODES = ((False, False), (False, True), (True, False), (True, True))  # (inverse, coset), the program's output order
LIMIT_KAKB, LIMIT_K_STORE = 70.0, 35.0


def _replay(kind, log_n, bmax, blob, tmp_path):
    assert os.path.exists(EXE), "tests/host/_ntt_pass_check not built (build() compiles it)"
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(blob)
    p = subprocess.run([EXE, kind, str(log_n), str(bmax), str(fin), str(fout)], capture_output=True, text=True, timeout=500)
    assert p.returncode == 0, (kind, log_n, bmax, p.stdout[-2000:], p.stderr[-3000:])
    stats = {k: float(v) for k, v in re.findall(r"(max_\w+) ([0-9.]+)", p.stdout)}
    assert set(stats) == {"max_kakb", "max_k_final_store", "max_k_col_store"}, p.stdout
    print(kind, log_n, bmax, p.stdout.strip())
    assert stats["max_kakb"] <= LIMIT_KAKB and max(stats["max_k_final_store"], stats["max_k_col_store"]) <= LIMIT_K_STORE
    return fout.read_bytes(), stats


def _first_diff(got, want):
    assert len(got) == len(want), (len(got), len(want))
    return next((i for i in range(len(got) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]), None)


def _check_ntt(co, log_n, bmax, cases, tmp_path):
    n = 1 << log_n
    blobs = [raw_fr_bytes(v) for _, v in cases]
    out, stats = _replay("ntt", log_n, bmax, b"".join(blobs), tmp_path)
    assert len(out) == 32 * n * 4 * len(cases)
    for ci, (name, _) in enumerate(cases):
        for mi, (inv, cs) in enumerate(MODES):
            got = out[32 * n * (4 * ci + mi):32 * n * (4 * ci + mi + 1)]
            want = co.ntt(blobs[ci], log_n, inv, cs, nthreads=co.ncpu())
            assert got == want, "pattern %s, log_n %d, bmax %d, inverse %d coset %d: first differing element %s" % (name, log_n, bmax, inv, cs, _first_diff(got, want))
            if name == "zeros":
                assert got == bytes(32 * n)
    return stats


@pytest.mark.parametrize("log_n", list(range(1, 13)))
def test_replay_of_one_and_two_pass_plans_equals_the_oracle(co, log_n, tmp_path):
    """1 .. 10: one pass with an odd and an even stage count; 11, 12: 6+5 and 6+6"""
    n = 1 << log_n
    _check_ntt(co, log_n, 10, V.named(n) + [("uniform", V.uniform(n))], tmp_path)


@pytest.mark.parametrize("part", range(3))
def test_replay_at_2p20_equals_the_oracle(co, part, tmp_path):
    """10+10: the full ten stages in both passes, the two-level inter-pass twiddle with every hi index.  Every pattern plus uniform, a third of the list per
    case (16 transforms = 210 M checked products each, spread over the program's threads)"""
    n = 1 << 20
    cases = V.named(n) + [("uniform", V.uniform(n))]
    assert len(cases) == 12
    _check_ntt(co, 20, 10, cases[part::3], tmp_path)


@pytest.mark.parametrize("log_n", [9, 12])
def test_replay_of_three_pass_plans_equals_the_oracle(co, log_n, tmp_path):
    """BZK_NTT_BMAX = 4 makes a three-pass plan of a small transform (3+3+3, 4+4+4): the middle pass in place and its single-level twiddle table"""
    n = 1 << log_n
    _check_ntt(co, log_n, 4, V.named(n) + [("uniform", V.uniform(n))], tmp_path)


@pytest.mark.parametrize("log_m", [5, 10, 11])
def test_replay_of_the_h_chain_equals_the_oracle(co, log_m, tmp_path):
    """NTT_INV_TO_COSET, NTT_FWD_RAW, NTT_FWD_RAW_S5 and NTT_INV_COSET_PW (the pointwise step in the first load), as ntt_h_chain strings them"""
    m = 1 << log_m
    cases = V.h_cases(m) + [("uniform", V.uniform(m, 1), V.uniform(m, 2), V.uniform(m - m // 3, 3) + [0] * (m // 3), False)]
    pad = lambda v: raw_fr_bytes(v) + bytes(32 * (m - len(v)))
    out, _ = _replay("h", log_m, 10, b"".join(pad(a) + pad(b) + pad(c) for _, a, b, c, _ in cases), tmp_path)
    assert len(out) == 32 * m * len(cases)
    for ci, (name, a, b, c, zero) in enumerate(cases):
        got = out[32 * m * ci:32 * m * ci + 32 * (m - 1)]
        want = co.groth16_h(pad(a), pad(b), pad(c), log_m, nthreads=co.ncpu())
        assert got == want, "h case %s, log_m %d: first differing coefficient %s" % (name, log_m, _first_diff(got, want))
        if zero:
            assert got == bytes(32 * (m - 1)), name
