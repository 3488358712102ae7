"""The phase-2 re-key on the GPU (bazuka_amd/csrc/rekey.hip: g1_scale_kernel): bzk_g1_scale_batch[_dev] against the ctx = NULL route and the oracle at
the sizes where a block can go wrong (a lone lane, a partial last wave, a partial last block) and across one staging round; bzk_params_rekey against
bzk_groth16_setup with delta * d, with the source handle left as it was; the file route and its verdict on the device."""
import random

import pytest
import torch

from bazuka_amd import lib as L
from oracle import pyref as pr_mod
from util import dev_bytes, fr_bytes, fr_list, r1cs_to_csr, synth_r1cs, to_dev

pytestmark = pytest.mark.gpu

R = pr_mod.R_MOD
N_MAX = 257
ROUND = 1 << 18  # rekey.hip SC_ROUND: the points of one staged round


def scalars():
    """the issue's table: 1, 2, r - 1, (r + 1) / 2, 2^128 - 1, 2^128, a value whose low 64 bits are zero, two seeded random values"""
    rnd = random.Random(20240)
    return [1, 2, R - 1, (R + 1) // 2, 2 ** 128 - 1, 2 ** 128, ((0x1234567890abcdef0fedcba987654321 << 64) % R) & ~(2 ** 64 - 1),
            rnd.randrange(R), rnd.randrange(R)]


def oracle_scaled(co, pts: bytes, k: int) -> bytes:
    out = []
    for i in range(len(pts) // 96):
        q = co.g1_mul(pts[96 * i:96 * i + 96] + b"\0", pr_mod.fr_to_canon_bytes(k))
        assert q[96] == 0
        out.append(q[:96])
    return b"".join(out)


@pytest.fixture(scope="module")
def reference(co):
    """(points, {k: the oracle's products of all N_MAX points}), computed once; every size below takes a prefix"""
    pts = co.g1_bases(7, 0, N_MAX)
    want = {k: oracle_scaled(co, pts, k) for k in scalars()}
    for k in scalars():
        assert L.g1_scale_batch(None, pts, pr_mod.fr_to_mont_bytes(k)) == (want[k], bytes(N_MAX))
    return pts, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_device_scale_against_host_route_and_oracle(bzk, reference, n):
    pts, want = reference
    mine = pts[:96 * n]
    for k in scalars():
        kb = pr_mod.fr_to_mont_bytes(k)
        assert bzk.g1_scale_batch(mine, kb) == (want[k][:96 * n], bytes(n)), k
        dp, di = to_dev(mine), to_dev(b"\7" * n)  # the _dev form, in place
        torch.cuda.synchronize()
        bzk.g1_scale_batch_dev(dp, n, kb, dp, di)
        assert dev_bytes(dp) == want[k][:96 * n] and dev_bytes(di) == bytes(n), k
    out, inf = bzk.g1_scale_batch(mine, pr_mod.fr_to_mont_bytes(0))
    assert out == bytes(96 * n) and inf == b"\1" * n
    dp, dq = to_dev(mine), to_dev(b"\7" * (96 * n))  # out of place, no flags
    torch.cuda.synchronize()
    bzk.g1_scale_batch_dev(dp, n, pr_mod.fr_to_mont_bytes(scalars()[7]), dq, None)
    assert dev_bytes(dq) == want[scalars()[7]][:96 * n] and dev_bytes(dp) == mine


def test_one_round_crossing(bzk, reference):
    """ONE host-pointer call of a round + 65 points: the second round's records, results and flags land behind the first's"""
    pts, want = reference
    k = scalars()[8]
    n = ROUND + 65
    reps, rest = divmod(n, 17)
    recs = pts[:96 * 17] * reps + pts[:96 * rest]
    out, inf = bzk.g1_scale_batch(recs, pr_mod.fr_to_mont_bytes(k))
    assert inf == bytes(n)
    assert out == want[k][:96 * 17] * reps + want[k][:96 * rest]


def test_arguments(bzk, reference):
    import ctypes as C
    pts, _ = reference
    lib = L.load_library()
    one = pr_mod.fr_to_mont_bytes(1)
    buf = C.create_string_buffer(b"\xa5" * 96, 96)
    assert lib.bzk_g1_scale_batch(bzk.h, None, 0, one, None, None) == 0
    assert lib.bzk_g1_scale_batch(bzk.h, pts, 1, R.to_bytes(32, "little"), buf, None) == -1 and buf.raw == b"\xa5" * 96
    assert lib.bzk_g1_scale_batch(bzk.h, None, 1, one, buf, None) == -1
    assert lib.bzk_g1_scale_batch_dev(None, None, 0, one, None, None) == -1  # the _dev form needs a context
    assert lib.bzk_g1_scale_batch_dev(bzk.h, None, 0, one, None, None) == 0
    assert lib.bzk_g1_scale_batch_dev(bzk.h, None, 2, one, None, None) == -1


# ---- a resident key
def _csr_bytes(r1):
    import array
    out = []
    for which in range(3):
        rp, col, val = array.array("I", [0]), array.array("I"), []
        for row in r1["rows"]:
            for v, c in row[which]:
                col.append(v)
                val.append(pr_mod.fr_to_mont_bytes(c))
            rp.append(len(col))
        out.append((len(r1["rows"]), rp.tobytes(), col.tobytes(), b"".join(val)))
    return out


def _circuit(co):
    r1 = synth_r1cs(30, seed=4242 + 30)  # the circuit of test_gpu_groth16.py::test_gpu_setup_matches_oracle_crs
    return r1, _csr_bytes(r1)


TOX = fr_list(5, 99)
D = random.Random(99001).randrange(1, R)


def test_resident_rekey_equals_setup_with_scaled_delta(bzk, co):
    r1, csr = _circuit(co)
    ph, _ = bzk.groth16_setup(csr, r1["n_in"], r1["n_aux"], fr_bytes(TOX))
    pw, vkw = bzk.groth16_setup(csr, r1["n_in"], r1["n_aux"], fr_bytes(TOX[:4] + [TOX[4] * D % R]))
    pn, vk870 = bzk.params_rekey(ph, pr_mod.fr_to_mont_bytes(D))
    for which in range(6):
        assert bzk.params_read(pn, which) == bzk.params_read(pw, which), which
    assert vk870 == vkw[:870] == bzk.params_read(pn, 0)
    for bad in (pr_mod.fr_to_mont_bytes(0), R.to_bytes(32, "little")):
        with pytest.raises(L.BzkError):
            bzk.params_rekey(ph, bad)
    for h in (ph, pw, pn):
        bzk.params_free(h)


def test_the_source_is_left_as_it_was(bzk, co):
    r1, csr = _circuit(co)
    A, B, Cm = r1cs_to_csr(co, r1)
    zb = fr_bytes(r1["z"])
    az, bz, cz = co.r1cs_eval(A, B, Cm, zb, nthreads=co.ncpu())
    r, s = fr_bytes(fr_list(2, 8))[:32], fr_bytes(fr_list(2, 8))[32:]
    ph, vk_old = bzk.groth16_setup(csr, r1["n_in"], r1["n_aux"], fr_bytes(TOX))
    proof_old = bzk.groth16_prove(ph, zb, az, bz, cz, r, s)  # the source's resident forms exist from here on
    was = [bzk.params_read(ph, which) for which in range(6)]
    pn, vk870 = bzk.params_rekey(ph, pr_mod.fr_to_mont_bytes(D))
    assert [bzk.params_read(ph, which) for which in range(6)] == was
    assert bzk.groth16_prove(ph, zb, az, bz, cz, r, s) == proof_old
    proof_new = bzk.groth16_prove(pn, zb, az, bz, cz, r, s)
    vk_new = vk870 + vk_old[870:]
    pub = fr_bytes(r1["z"][1:r1["n_in"]])
    assert L.groth16_verify(vk_new, pub, proof_new) and not L.groth16_verify(vk_old, pub, proof_new)
    assert L.groth16_verify(vk_old, pub, proof_old) and not L.groth16_verify(vk_new, pub, proof_old)
    assert bzk.groth16_prove(ph, zb, az, bz, cz, r, s) == proof_old
    bzk.params_free(pn)
    bzk.params_free(ph)


def test_file_route_on_the_device(bzk):
    r1 = synth_r1cs(6, n_in=3, seed=77)  # the circuit of tests/test_bellman_params_cpu.py
    p = pr_mod.groth16_setup(pr_mod.R1CS(r1["n_in"], r1["n_aux"], r1["rows"][:-r1["n_in"]]), 11111, 22222, 33333, 44444, 55555)
    vk = {k: p[k] for k in ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "delta_g1", "delta_g2", "ic")}
    before = pr_mod.bellman_params_bytes(vk, p["h"], p["l"], p["a"], p["b_g1"], p["b_g2"])
    db = pr_mod.fr_to_mont_bytes(D)
    after = bzk.bellman_params_rekey(before, db)
    assert after == L.bellman_params_rekey(None, before, db)
    seed = bytes(range(32))
    assert bzk.bellman_params_rekey_check(before, after, seed) == (1, (0, 0, 0, 0))
    A = L.bellman_params_decode(after)
    swapped = L.bellman_params_encode(A["vk"], A["ic"], A["h"][96:192] + A["h"][:96] + A["h"][192:], A["l"], A["a"], A["b_g1"], A["b_g2"])
    verdict, report = bzk.bellman_params_rekey_check(before, swapped, seed)
    assert verdict == 0 and report[0] == 2
    assert L.bellman_params_rekey_check(None, before, swapped, seed) == (verdict, report)
