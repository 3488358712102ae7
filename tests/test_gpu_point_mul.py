"""n points times n scalars on the GPU (bazuka_amd/csrc/pmul.hip: g1_pmul_kernel, g2_pmul_kernel and the preparation kernels): bzk_g1_mul_batch[_dev]
and bzk_g2_mul_batch[_dev] against the ctx = NULL route and the oracle at the sizes where a block can go wrong (a lone lane, a partial wave, a partial
last block), with the scalar table mixed inside every wavefront - a multiplier that took its bit from one lane for the whole wave fails every size
above 1; one wave with a single non-zero scalar; the powers form from a high start; one staging-round crossing; the arguments."""
import pytest
import torch

import point_mul_cases as pc
from bazuka_amd import lib as L
from oracle import pyref as pr
from util import dev_bytes, to_dev

pytestmark = pytest.mark.gpu

R = pr.R_MOD
ROUND = 1 << 18  # pmul.hip PM_ROUND: the points of one staged round
GROUPS = ("g1", "g2")


@pytest.fixture(scope="module")
def reference():
    """{group: (points, scalars, products, flags)}; the ctx = NULL route agrees with the oracle on all N_MAX lanes"""
    out = {}
    for g in GROUPS:
        pts, ks, want, winf = pc.reference(g)
        assert L.mul_batch(None, g, pts, pc.mont(ks)) == (want, winf)
        out[g] = (pts, ks, want, winf)
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("group", GROUPS)
def test_device_products_against_host_route_and_oracle(bzk, reference, group, n):
    pts, ks, want, winf = reference[group]
    sz = pc.SIZE[group]
    mine, want, winf = pts[:sz * n], want[:sz * n], winf[:n]
    km, kc = pc.mont(ks[:n]), pc.canon(ks[:n])
    assert bzk.mul_batch(group, mine, km) == (want, winf)
    assert bzk.mul_batch(group, mine, kc, canonical=True) == (want, winf)
    dp, dk, di = to_dev(mine), to_dev(km), to_dev(b"\7" * n)  # the _dev form, in place, with flags
    torch.cuda.synchronize()
    bzk.mul_batch_dev(group, dp, dk, n, dp, di)
    assert dev_bytes(dp) == want and dev_bytes(di) == winf and dev_bytes(dk) == km
    dp, dk, dq = to_dev(mine), to_dev(kc), to_dev(b"\7" * (sz * n))  # out of place, canonical scalars, no flags
    torch.cuda.synchronize()
    bzk.mul_batch_dev(group, dp, dk, n, dq, None, canonical=True)
    assert dev_bytes(dq) == want and dev_bytes(dp) == mine


@pytest.mark.parametrize("group", GROUPS)
def test_one_lane_of_a_wave_has_a_scalar(bzk, reference, group):
    """lane 37 alone: every other lane of the wave must come out as the identity, and lane 37 as its own product"""
    pts, ks, _, _ = reference[group]
    sz = pc.SIZE[group]
    k = pc.scalar_table()[-1]
    mine = pts[:sz * 64]
    one = pc.oracle_products(group, pts[sz * 37:sz * 38], [k])[0]
    want = (bytes(sz * 37) + one + bytes(sz * 26), b"\1" * 37 + b"\0" + b"\1" * 26)
    assert bzk.mul_batch(group, mine, pc.mont([0] * 37 + [k] + [0] * 26)) == want
    # and the other way round: lane 37 alone has none
    ks1 = [k] * 37 + [0] + [k] * 26
    assert bzk.mul_batch(group, mine, pc.mont(ks1)) == L.mul_batch(None, group, mine, pc.mont(ks1))


@pytest.mark.parametrize("group", GROUPS)
def test_powers_from_a_high_start(bzk, reference, group):
    pts, _, _, _ = reference[group]
    sz, n, start = pc.SIZE[group], 70, 2 ** 18 - 3
    c, s = 0x1234567890abcdef1122334455667788 * 0x10001 % R, 0x0fedcba987654321aabbccddeeff0011 ** 2 % R
    mine = pts[:sz * n]
    want = pc.oracle_products(group, mine, [c * pow(s, start + i, R) % R for i in range(n)])
    cb, sb = pr.fr_to_mont_bytes(c), pr.fr_to_mont_bytes(s)
    assert L.mul_powers(None, group, mine, cb, sb, start) == want
    dp, di = to_dev(mine), to_dev(b"\7" * n)
    torch.cuda.synchronize()
    bzk.mul_powers_dev(group, dp, n, cb, sb, start, dp, di)
    assert (dev_bytes(dp), dev_bytes(di)) == want
    assert bzk.mul_powers(group, mine, cb, sb, start) == want


def test_one_round_crossing(bzk, reference):
    """ONE host-pointer call of a round + 65 points: the second round's records, scalars, results and flags land behind the first's"""
    pts, ks, want, winf = reference["g1"]
    n = ROUND + 65
    reps, rest = divmod(n, 17)
    km = pc.mont(ks[:17])
    recs = pts[:96 * 17] * reps + pts[:96 * rest]
    out, inf = bzk.mul_batch("g1", recs, km * reps + km[:32 * rest])
    assert inf == winf[:17] * reps + winf[:rest]
    assert out == want[:96 * 17] * reps + want[:96 * rest]


def test_arguments(bzk, reference):
    import ctypes as C
    lib = L.load_library()
    one = pr.fr_to_mont_bytes(1)
    for group in GROUPS:
        pts = reference[group][0]
        sz = pc.SIZE[group]
        batch, batch_dev = {"g1": (lib.bzk_g1_mul_batch, lib.bzk_g1_mul_batch_dev), "g2": (lib.bzk_g2_mul_batch, lib.bzk_g2_mul_batch_dev)}[group]
        powers, powers_dev = {"g1": (lib.bzk_g1_mul_powers, lib.bzk_g1_mul_powers_dev), "g2": (lib.bzk_g2_mul_powers, lib.bzk_g2_mul_powers_dev)}[group]
        fill = b"\xa5" * (2 * sz)
        buf = C.create_string_buffer(fill, 2 * sz)
        assert batch(bzk.h, None, None, 0, 0, None, None) == 0
        assert batch(bzk.h, pts, one + R.to_bytes(32, "little"), 2, 0, buf, None) == -1 and buf.raw == fill
        assert batch(bzk.h, None, one, 1, 0, buf, None) == -1 and batch(bzk.h, pts, None, 1, 0, buf, None) == -1
        assert batch(bzk.h, pts, one, 1, 0, None, None) == -1
        assert powers(bzk.h, pts, 2, R.to_bytes(32, "little"), one, 0, buf, None) == -1 and buf.raw == fill
        assert powers(bzk.h, pts, 2, one, None, 0, buf, None) == -1
        assert batch_dev(bzk.h, None, None, 0, 0, None, None) == 0 and powers_dev(bzk.h, None, 0, one, one, 0, None, None) == 0
        assert batch_dev(bzk.h, None, None, 2, 0, None, None) == -1 and powers_dev(bzk.h, None, 2, one, one, 0, None, None) == -1
        # scalars in device memory: the one bad row is found before the first record is written
        n = 70
        dp, dq = to_dev(pts[:sz * n]), to_dev(b"\7" * (sz * n))
        dk = to_dev(one * 69 + R.to_bytes(32, "little"))
        torch.cuda.synchronize()
        assert batch_dev(bzk.h, dp.data_ptr(), dk.data_ptr(), n, 0, dq.data_ptr(), None) == -1
        assert dev_bytes(dq) == b"\7" * (sz * n)
        assert batch_dev(bzk.h, dp.data_ptr() + 1, dk.data_ptr(), n, 0, dq.data_ptr(), None) == -1  # 4-byte alignment
