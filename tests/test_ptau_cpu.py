"""The powers-of-tau accumulator on host threads (ctx = NULL): bzk_ptau_init, bzk_ptau_contribute against the oracle's multiples of the generators, two
contributions against one with the product secrets, the verdicts of bzk_ptau_check on a true step and on forgeries, the refusals, and the tie to the
existing key path: the h query and the head of pyref's groth16_setup(tau, alpha, beta, 1, 1) read off the accumulator of the same secrets."""
import ctypes as C
import random

import pytest

import point_mul_cases as pc
import subgroup_cases
from bazuka_amd import lib as L
from oracle import coracle as co
from oracle import pyref as pr
from util import synth_r1cs

R = pr.R_MOD
LOG_M = 3
_rnd = random.Random(31337)
TAU, ALPHA, BETA = (_rnd.randrange(1, R) for _ in range(3))
TAU2, ALPHA2, BETA2 = (_rnd.randrange(1, R) for _ in range(3))
SEEDS = [bytes(range(32)), b"\x5a" * 32]


def secrets(*s) -> bytes:
    return b"".join(pr.fr_to_mont_bytes(x) for x in s)


@pytest.fixture(scope="module")
def trivial():
    return L.ptau_init(LOG_M)


@pytest.fixture(scope="module")
def first(trivial):
    return L.ptau_contribute(None, trivial, secrets(TAU, ALPHA, BETA))


@pytest.fixture(scope="module")
def second(first):
    return L.ptau_contribute(None, first[0], secrets(TAU2, ALPHA2, BETA2))


def test_size_and_init(trivial):
    lay, size = pc.layout(LOG_M)
    assert L.ptau_size(LOG_M) == size == len(trivial)
    assert [L.ptau_size(x) for x in (0, 25, 2 ** 31)] == [0, 0, 0] and L.ptau_size(24) == pc.layout(24)[1]
    assert trivial[:16] == b"BZKPTAU1" + (LOG_M).to_bytes(4, "little") + bytes(4)
    for name, (off, cnt, sz) in lay.items():
        gen = (co.g1_generator() if sz == 96 else co.g2_generator())[:sz]
        assert trivial[off:off + cnt * sz] == gen * cnt, name
    assert trivial == pc.oracle_accumulator(LOG_M, 1, 1, 1)


def test_contribution_equals_the_oracle(first, second):
    assert first == (pc.oracle_accumulator(LOG_M, TAU, ALPHA, BETA), pc.oracle_key(TAU, ALPHA, BETA))
    # two contributions are one with the product secrets; the key is the second contribution's own
    assert second[0] == pc.oracle_accumulator(LOG_M, TAU * TAU2 % R, ALPHA * ALPHA2 % R, BETA * BETA2 % R)
    assert second[1] == pc.oracle_key(TAU2, ALPHA2, BETA2)


@pytest.mark.parametrize("seed", SEEDS)
def test_true_steps_pass(trivial, first, second, seed):
    ok = (1, (0, 0, 0, 0))
    assert L.ptau_check(None, None, None, trivial, seed) == ok
    assert L.ptau_check(None, None, None, first[0], seed) == ok
    assert L.ptau_check(None, trivial, first[1], first[0], seed) == ok
    assert L.ptau_check(None, first[0], second[1], second[0], seed) == ok
    assert L.ptau_check(None, None, None, second[0], seed) == ok


def forgeries(first, second):
    """[(name, before, key, forged after, the array the verdict must name)] on the step first -> second"""
    before, (after, key) = first[0], second
    e = lambda name, i: pc.entry(after, LOG_M, name, i)
    put = lambda name, i, rec: pc.with_entry(after, LOG_M, name, i, rec)
    other = L.ptau_contribute(None, before, secrets(TAU, ALPHA2, BETA2))  # a step by another tau
    lay, _ = pc.layout(LOG_M)
    out = []
    swap = lambda name, i, j: pc.with_entry(put(name, i, e(name, j)), LOG_M, name, j, e(name, i))
    out.append(("tau_g1[2] and tau_g1[3] swapped", swap("tau_g1", 2, 3), 1))
    out.append(("alpha_g1[2] replaced by another subgroup point", put("alpha_g1", 2, e("beta_g1", 2)), 3))
    off, cnt, sz = lay["tau_g2"]
    # tau_g1's relation is stated against tau_g2[1], so it is the first to fail when tau_g2 is another tau's
    out.append(("tau_g2 taken from another tau", after[:off] + other[0][off:off + cnt * sz] + after[off + cnt * sz:], 1))
    out.append(("tau_g2[2] and tau_g2[3] swapped", swap("tau_g2", 2, 3), 2))
    out.append(("beta_g1 shifted by one power", put("beta_g1", 5, e("beta_g1", 4)), 4))
    out.append(("a wrong beta_g2", put("beta_g2", 0, e("tau_g2", 1)), 5))
    torsion = subgroup_cases.outside_point("g1")
    mixed = co.g1_add(e("tau_g1", 4) + b"\0", torsion + b"\0")
    assert mixed[96] == 0
    out.append(("tau_g1[4] with a cofactor component", put("tau_g1", 4, mixed[:96]), 1))
    out.append(("a truncated blob", after[:-96], 0))
    return [(name, before, key, forged, array) for name, forged, array in out] + [("a key of other secrets", before, other[1], after, 6)]


@pytest.mark.parametrize("seed", SEEDS)
def test_forgeries_fail_with_their_array(first, second, seed):
    cases = forgeries(first, second)
    assert len(cases) == 9
    for name, before, key, forged, array in cases:
        verdict, report = L.ptau_check(None, before, key, forged, seed)
        assert verdict == 0 and report[0] == array and report[3] == 0, (name, verdict, report)
        if "cofactor" in name:
            assert report == (1, 4, 0, 0)  # on the curve, outside the subgroup
        if array not in (0, 6):  # the same verdict without the step
            assert L.ptau_check(None, None, None, forged, seed) == (verdict, report), name
    # an identity entry is refused by the subgroup pass: no finite curve point
    after = second[0]
    assert L.ptau_check(None, None, None, pc.with_entry(after, LOG_M, "alpha_g1", 7, bytes(96)), seed) == (0, (3, 7, 2, 0))
    # the generators are compared byte for byte: an accumulator scaled by a constant keeps every ratio
    scaled = L.mul_batch(None, "g1", after[16:16 + 96 * 15], pc.mont([2] * 15))[0]
    assert L.ptau_check(None, None, None, after[:16] + scaled + after[16 + 96 * 15:], seed)[1][:2] == (1, 0)
    # before of another size
    assert L.ptau_check(None, L.ptau_init(2), second[1], after, seed) == (0, (0, 1, 0, 0))


def test_refusals(trivial):
    lib = L.load_library()
    n = len(trivial)
    fill = b"\xa5" * (n + 64)
    buf, key = C.create_string_buffer(fill, n + 64), C.create_string_buffer(b"\xa5" * 576, 576)
    good = secrets(TAU, ALPHA, BETA)
    bad_secrets = [secrets(0, ALPHA, BETA), secrets(TAU, 0, BETA), secrets(TAU, ALPHA, 0), good[:64] + R.to_bytes(32, "little")]
    for s in bad_secrets:
        assert lib.bzk_ptau_contribute(None, trivial, n, s, buf, n, key) == -1
    assert lib.bzk_ptau_contribute(None, trivial, n, good, buf, n - 1, key) == -1          # cap one byte short
    assert lib.bzk_ptau_contribute(None, trivial, n - 1, good, buf, n, key) == -1          # a blob that does not parse
    assert lib.bzk_ptau_contribute(None, b"X" + trivial[1:], n, good, buf, n, key) == -1
    assert lib.bzk_ptau_contribute(None, trivial[:8] + (25).to_bytes(4, "little") + trivial[12:], n, good, buf, n, key) == -1
    assert lib.bzk_ptau_contribute(None, trivial, n, good, buf, n, None) == -1
    assert buf.raw == fill and key.raw == b"\xa5" * 576
    assert lib.bzk_ptau_init(LOG_M, buf, n - 1) == -1 and lib.bzk_ptau_init(0, buf, n) == -1 and lib.bzk_ptau_init(LOG_M, None, n) == -1
    assert buf.raw == fill
    assert lib.bzk_ptau_contribute(None, trivial, n, good, buf, n, key) == 0 and buf.raw[n:] == b"\xa5" * 64  # nothing beyond the blob
    report = (C.c_uint64 * 4)()
    seed = bytes(32)
    assert lib.bzk_ptau_check(None, trivial, n, None, trivial, n, seed, report) == -1     # before without a key
    assert lib.bzk_ptau_check(None, None, 0, key, trivial, n, seed, report) == -1         # a key without before
    assert lib.bzk_ptau_check(None, None, 0, None, None, n, seed, report) == -1


def test_in_place_contribution(trivial, first):
    n = len(trivial)
    buf, key = C.create_string_buffer(trivial, n), C.create_string_buffer(576)
    assert L.load_library().bzk_ptau_contribute(None, buf, n, secrets(TAU, ALPHA, BETA), buf, n, key) == 0
    assert (buf.raw, key.raw) == first


def test_the_accumulator_holds_the_key_path_s_points():
    """log_m = 4: the circuit of test_file_route_on_the_device (6 rows + 3 inputs).  With delta = gamma = 1 the h query of groth16_setup is
    (tau^m - 1) tau^i G1 = tau_g1[i + m] - tau_g1[i], and alpha_g1, beta_g1, beta_g2 of the head are entry 0 of their arrays"""
    r1 = synth_r1cs(6, n_in=3, seed=77)
    p = pr.groth16_setup(pr.R1CS(r1["n_in"], r1["n_aux"], r1["rows"][:-r1["n_in"]]), TAU, ALPHA, BETA, 1, 1)
    m = len(p["h"]) + 1
    assert m == 16  # the domain, from the length of h
    acc, _ = L.ptau_contribute(None, L.ptau_init(4), secrets(TAU, ALPHA, BETA))
    e = lambda name, i: pc.entry(acc, 4, name, i)
    minus_one = pr.fr_to_canon_bytes(R - 1)
    for i in range(m - 1):
        neg = co.g1_mul(e("tau_g1", i) + b"\0", minus_one)
        assert co.g1_add(e("tau_g1", i + m) + b"\0", neg) == pr.g1_to_bytes(p["h"][i]), i
    assert e("alpha_g1", 0) + b"\0" == pr.g1_to_bytes(p["alpha_g1"])
    assert e("beta_g1", 0) + b"\0" == pr.g1_to_bytes(p["beta_g1"])
    assert e("beta_g2", 0) + b"\0" == pr.g2_to_bytes(p["beta_g2"])
