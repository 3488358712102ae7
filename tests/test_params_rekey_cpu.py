"""The phase-2 re-key on host threads (ctx = NULL): bzk_g1_scale_batch against the oracle's scalar multiplication, bzk_bellman_params_rekey against
the oracle's setup with delta * d (the re-key of setup(tau, alpha, beta, gamma, delta) by d IS setup(tau, alpha, beta, gamma, delta * d), byte for
byte), the verdicts of bzk_bellman_params_rekey_check on a true re-key and on six forgeries, and the refusals."""
import ctypes as C
import os
import random
import subprocess

import pytest

from bazuka_amd import lib as L
from oracle import coracle as co
from oracle import pyref as pr
from util import synth_r1cs

R = pr.R_MOD
P = pr.P_MOD
TOXIC = (11111, 22222, 33333, 44444, 55555)


def scalars():
    """the issue's table: 1, 2, r - 1, (r + 1) / 2, 2^128 - 1, 2^128, a value whose low 64 bits are zero, two seeded random values"""
    rnd = random.Random(20240)
    return [1, 2, R - 1, (R + 1) // 2, 2 ** 128 - 1, 2 ** 128, ((0x1234567890abcdef0fedcba987654321 << 64) % R) & ~(2 ** 64 - 1),
            rnd.randrange(R), rnd.randrange(R)]


def oracle_scaled(pts: bytes, k: int) -> bytes:
    out = []
    for i in range(len(pts) // 96):
        q = co.g1_mul(pts[96 * i:96 * i + 96] + b"\0", pr.fr_to_canon_bytes(k))
        assert q[96] == 0
        out.append(q[:96])
    return b"".join(out)


POINTS = co.g1_bases(7, 0, 37)


@pytest.mark.parametrize("k", scalars())
def test_scale_against_the_oracle(k):
    out, inf = L.g1_scale_batch(None, POINTS, pr.fr_to_mont_bytes(k))
    assert inf == bytes(37)
    assert out == oracle_scaled(POINTS, k)
    if k == R - 1:  # -P: x as it was, y negated (Montgomery limbs of p - y)
        for i in range(37):
            assert out[96 * i:96 * i + 48] == POINTS[96 * i:96 * i + 48]
            y = int.from_bytes(POINTS[96 * i + 48:96 * i + 96], "little")
            assert int.from_bytes(out[96 * i + 48:96 * i + 96], "little") == P - y


def test_scale_by_zero_and_argument_handling():
    out, inf = L.g1_scale_batch(None, POINTS, pr.fr_to_mont_bytes(0))
    assert out == bytes(96 * 37) and inf == b"\1" * 37
    assert L.g1_scale_batch(None, out[:96 * 3], pr.fr_to_mont_bytes(5)) == (bytes(96 * 3), b"\1" * 3)  # the identity as this call writes it
    assert L.g1_scale_batch(None, b"", pr.fr_to_mont_bytes(3)) == (b"", b"")
    lib = L.load_library()
    buf = C.create_string_buffer(b"\xa5" * 96, 96)
    for bad in (R.to_bytes(32, "little"), b"\xff" * 32):  # limbs not below r: refused, nothing written
        assert lib.bzk_g1_scale_batch(None, POINTS, 1, bad, buf, None) == -1
        assert buf.raw == b"\xa5" * 96
    assert lib.bzk_g1_scale_batch(None, None, 1, pr.fr_to_mont_bytes(1), buf, None) == -1
    assert lib.bzk_g1_scale_batch(None, POINTS, 1, pr.fr_to_mont_bytes(1), None, None) == -1
    assert lib.bzk_g1_scale_batch(None, POINTS, 1, pr.fr_to_mont_bytes(1), buf, None) == 0 and buf.raw == POINTS[:96]  # inf_out may be NULL


def test_device_field_instantiation_on_the_cpu(tmp_path):
    """scale_point over the device's 28-bit field with the bound assertions on (tests/host/_scale_check), every scalar of the table and zero"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "_scale_check")
    assert os.path.exists(exe), "tests/host/_scale_check not built (build() compiles it)"
    f = tmp_path / "pts.bin"
    f.write_bytes(POINTS[:96 * 5])
    for k in scalars() + [0]:
        p = subprocess.run([exe, str(f), pr.fr_to_mont_bytes(k).hex()], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        want = oracle_scaled(POINTS[:96 * 5], k) if k else bytes(96 * 5)
        assert p.stdout.split() == ["inf", ("1" if k == 0 else "0") * 5, "out", want.hex()], k


# ---- the file route
_R1 = synth_r1cs(6, n_in=3, seed=77)
_CS = pr.R1CS(_R1["n_in"], _R1["n_aux"], _R1["rows"][:-_R1["n_in"]])


def blob_of(p) -> bytes:
    vk = {k: p[k] for k in ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "delta_g1", "delta_g2", "ic")}
    return pr.bellman_params_bytes(vk, p["h"], p["l"], p["a"], p["b_g1"], p["b_g2"])


@pytest.fixture(scope="module")
def before():
    return blob_of(pr.groth16_setup(_CS, *TOXIC))


D1, D2 = random.Random(77001).randrange(1, R), random.Random(77002).randrange(1, R)


@pytest.fixture(scope="module")
def after(before):
    return L.bellman_params_rekey(None, before, pr.fr_to_mont_bytes(D1))


@pytest.mark.parametrize("d", [1, R - 1, D1])
def test_file_rekey_equals_setup_with_scaled_delta(before, d):
    got = L.bellman_params_rekey(None, before, pr.fr_to_mont_bytes(d))
    t, a, b, g, dl = TOXIC
    assert got == blob_of(pr.groth16_setup(_CS, t, a, b, g, dl * d % R))
    if d == 1:
        assert got == before
    n = C.c_uint64(0)
    assert L.load_library().bzk_bellman_params_rekey(None, before, len(before), pr.fr_to_mont_bytes(d), None, 0, C.byref(n)) == 0
    assert n.value == len(got) == len(before)


def _enc(d) -> bytes:
    return L.bellman_params_encode(d["vk"], d["ic"], d["h"], d["l"], d["a"], d["b_g1"], d["b_g2"])


def forgeries(before: bytes, after: bytes):
    """[(name, forged `after`, the array the verdict must name)]"""
    A = L.bellman_params_decode(after)
    A2 = L.bellman_params_decode(L.bellman_params_rekey(None, before, pr.fr_to_mont_bytes(D2)))
    rec = lambda b, i: b[96 * i:96 * i + 96]
    put = lambda b, i, v: b[:96 * i] + v + b[96 * i + 96:]
    out = []
    out.append(("h'[0] and h'[1] swapped", _enc(dict(A, h=rec(A["h"], 1) + rec(A["h"], 0) + A["h"][192:])), 2))
    plus_g = co.g1_add(rec(A["l"], 2) + b"\0", co.g1_generator())
    assert plus_g[96] == 0
    out.append(("l'[2] + G1", _enc(dict(A, l=put(A["l"], 2, plus_g[:96]))), 3))
    assert rec(A["a"], 0) != rec(A["a"], 1)
    out.append(("a[0] replaced by a[1]", _enc(dict(A, a=put(A["a"], 0, rec(A["a"], 1)))), 4))
    out.append(("l scaled by another d", _enc(dict(A, l=A2["l"])), 3))
    out.append(("delta_g1 from d, delta_g2 from d2", _enc(dict(A, vk=A["vk"][:677] + A2["vk"][677:])), 0))
    out.append(("one h entry dropped", _enc(dict(A, h=A["h"][:-96])), 7))
    return out


@pytest.mark.parametrize("seed", [bytes(range(32)), b"\x5a" * 32])
def test_verdicts(before, after, seed):
    assert L.bellman_params_rekey_check(None, before, after, seed) == (1, (0, 0, 0, 0))
    cases = forgeries(before, after)
    assert len(cases) == 6
    for name, forged, array in cases:
        verdict, report = L.bellman_params_rekey_check(None, before, forged, seed)
        assert verdict == 0 and report[0] == array, (name, verdict, report)


def test_refusals(before):
    lib = L.load_library()
    with pytest.raises(L.BzkError):
        L.bellman_params_rekey(None, before, pr.fr_to_mont_bytes(0))
    with pytest.raises(L.BzkError):
        L.bellman_params_rekey(None, before, R.to_bytes(32, "little"))
    with pytest.raises(L.BzkError):
        L.bellman_params_rekey(None, before[:-1], pr.fr_to_mont_bytes(D1))
    n = len(before)
    buf = C.create_string_buffer(b"\xa5" * (n + 64), n + 64)
    assert lib.bzk_bellman_params_rekey(None, before, n, pr.fr_to_mont_bytes(D1), buf, n - 1, None) == -1  # cap one byte short
    assert buf.raw == b"\xa5" * (n + 64)
    for bad in (pr.fr_to_mont_bytes(0), R.to_bytes(32, "little")):
        assert lib.bzk_bellman_params_rekey(None, before, n, bad, buf, n, None) == -1
        assert buf.raw == b"\xa5" * (n + 64)
    assert lib.bzk_bellman_params_rekey(None, before, n, pr.fr_to_mont_bytes(D1), buf, n, None) == 0
    assert buf.raw[n:] == b"\xa5" * 64  # nothing beyond cap
