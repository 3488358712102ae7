"""n points times n scalars on host threads (ctx = NULL): bzk_g1_mul_batch / bzk_g2_mul_batch on the scalar table of tests/point_mul_cases.py against the
oracle's multiplications byte for byte, the powers forms against g1_mul(P_i, c s^(start + i)), the refusals, and the per-point function in its
device-field instantiation with the bound assertions on (tests/host/_pmul_check, a child process)."""
import ctypes as C
import os
import subprocess

import pytest

import point_mul_cases as pc
from bazuka_amd import lib as L
from oracle import pyref as pr

R, P = pr.R_MOD, pr.P_MOD
N = 37
GROUPS = ("g1", "g2")


@pytest.mark.parametrize("group", GROUPS)
def test_mul_batch_against_the_oracle(group):
    pts, ks, want, winf = pc.reference(group)
    sz = pc.SIZE[group]
    got = L.mul_batch(None, group, pts[:sz * N], pc.mont(ks[:N]))
    assert got == (want[:sz * N], winf[:N])
    assert L.mul_batch(None, group, pts[:sz * N], pc.canon(ks[:N]), canonical=True) == got
    assert set(ks[:N]) == set(pc.scalar_table())  # 37 lanes meet every entry of the table
    assert [i for i in range(N) if winf[i]] == [i for i in range(N) if ks[i] == 0]


@pytest.mark.parametrize("group", GROUPS)
def test_minus_one_negates_y(group):
    sz = pc.SIZE[group]
    pts = pc.points(group, 5)
    out, inf = L.mul_batch(None, group, pts, pc.mont([R - 1] * 5))
    assert inf == bytes(5)
    half = sz // 2
    for i in range(5):
        rec, got = pts[sz * i:sz * (i + 1)], out[sz * i:sz * (i + 1)]
        assert got[:half] == rec[:half]
        for j in range(half, sz, 48):  # every base-field limb string of y: Montgomery limbs of p - y
            assert int.from_bytes(got[j:j + 48], "little") == P - int.from_bytes(rec[j:j + 48], "little")


@pytest.mark.parametrize("group", GROUPS)
def test_identity_records_and_empty_calls(group):
    sz = pc.SIZE[group]
    pts = pc.points(group, 3)
    recs = pts[:sz] + bytes(sz) + pts[2 * sz:]
    out, inf = L.mul_batch(None, group, recs, pc.mont([5, 5, 5]))
    assert inf == b"\0\1\0" and out[sz:2 * sz] == bytes(sz)
    assert out[:sz] == pc.oracle_products(group, pts[:sz], [5])[0]
    assert L.mul_batch(None, group, b"", b"") == (b"", b"")
    assert L.mul_powers(None, group, b"", pr.fr_to_mont_bytes(1), pr.fr_to_mont_bytes(2)) == (b"", b"")


@pytest.mark.parametrize("group", GROUPS)
def test_refusals_leave_the_output_untouched(group):
    lib = L.load_library()
    sz = pc.SIZE[group]
    pts = pc.points(group, 2)
    batch = {"g1": lib.bzk_g1_mul_batch, "g2": lib.bzk_g2_mul_batch}[group]
    powers = {"g1": lib.bzk_g1_mul_powers, "g2": lib.bzk_g2_mul_powers}[group]
    fill = b"\xa5" * (2 * sz)
    buf = C.create_string_buffer(fill, 2 * sz)
    one = pr.fr_to_mont_bytes(1)
    for bad in (R.to_bytes(32, "little"), b"\xff" * 32):  # limbs not below r, in the second row: refused before the first is written
        for flags in (0, L.BZK_F_CANONICAL):
            assert batch(None, pts, one + bad, 2, flags, buf, None) == -1 and buf.raw == fill
        assert powers(None, pts, 2, bad, one, 0, buf, None) == -1 and buf.raw == fill
        assert powers(None, pts, 2, one, bad, 0, buf, None) == -1 and buf.raw == fill
    assert batch(None, None, one + one, 2, 0, buf, None) == -1
    assert batch(None, pts, None, 2, 0, buf, None) == -1
    assert batch(None, pts, one + one, 2, 0, None, None) == -1
    assert powers(None, pts, 2, None, one, 0, buf, None) == -1 and powers(None, pts, 2, one, None, 0, buf, None) == -1
    assert powers(None, None, 2, one, one, 0, buf, None) == -1 and powers(None, pts, 2, one, one, 0, None, None) == -1
    assert powers(None, pts, 2, one, one, 2 ** 64 - 1, buf, None) == -1  # start + n passes 2^64
    assert buf.raw == fill
    assert batch(None, None, None, 0, 0, None, None) == 0 and powers(None, None, 0, one, one, 0, None, None) == 0
    for dev in (lib.bzk_g1_mul_batch_dev, lib.bzk_g2_mul_batch_dev):  # the _dev forms need a context
        assert dev(None, None, None, 0, 0, None, None) == -1
    for dev in (lib.bzk_g1_mul_powers_dev, lib.bzk_g2_mul_powers_dev):
        assert dev(None, None, 0, one, one, 0, None, None) == -1
    assert batch(None, pts, one + one, 2, 0, buf, None) == 0 and buf.raw == pts  # inf_out may be NULL


C_S = (0x1234567890abcdef1122334455667788 * 0x10001 % R, 0x0fedcba987654321aabbccddeeff0011 ** 2 % R)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("start", [0, 5, 2 ** 18 - 3])
def test_mul_powers_against_the_oracle(group, start):
    c, s = C_S
    n = 9
    pts = pc.points(group, n)
    want = pc.oracle_products(group, pts, [c * pow(s, start + i, R) % R for i in range(n)])
    assert L.mul_powers(None, group, pts, pr.fr_to_mont_bytes(c), pr.fr_to_mont_bytes(s), start) == want
    assert L.mul_powers(None, group, pts, pr.fr_to_mont_bytes(0), pr.fr_to_mont_bytes(s), start) == (bytes(len(pts)), b"\1" * n)


@pytest.mark.parametrize("group", GROUPS)
def test_device_field_instantiation_on_the_cpu(tmp_path, group):
    """mul_point over the device's 28-bit field with the bound assertions on: every entry of the table on its own point, an identity record, and the
    powers form's scalars"""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "_pmul_check")
    assert os.path.exists(exe), "tests/host/_pmul_check not built (build() compiles it)"
    pts, ks, want, winf = pc.reference(group)
    sz = pc.SIZE[group]
    n = len(pc.scalar_table()) + 1
    recs = pts[:sz * (n - 1)] + bytes(sz)
    (tmp_path / "pts.bin").write_bytes(recs)
    (tmp_path / "sc.bin").write_bytes(pc.mont(ks[:n - 1] + [3]))
    p = subprocess.run([exe, group, str(tmp_path / "pts.bin"), "scalars", str(tmp_path / "sc.bin")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert p.stdout.split() == ["inf", "".join(str(b) for b in winf[:n - 1]) + "1", "out", (want[:sz * (n - 1)] + bytes(sz)).hex()]
    c, s = C_S
    start = 2 ** 18 - 3
    (tmp_path / "few.bin").write_bytes(pts[:sz * 4])
    p = subprocess.run([exe, group, str(tmp_path / "few.bin"), "powers", pr.fr_to_mont_bytes(c).hex(), pr.fr_to_mont_bytes(s).hex(), str(start)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out, inf = pc.oracle_products(group, pts[:sz * 4], [c * pow(s, start + i, R) % R for i in range(4)])
    assert p.stdout.split() == ["inf", "0000", "out", out.hex()]
