"""The powers-of-tau accumulator with a context: bzk_ptau_contribute (five powers calls on the device) and bzk_ptau_check (device MSMs, device subgroup
checks) at log_m = 3 and 8 against the ctx = NULL route - the same bytes, verdicts and reports on a true step and on a forgery - and the tie to
bzk_groth16_setup on the device with toxic = tau | alpha | beta | 1 | 1."""
import array
import random

import pytest

import point_mul_cases as pc
from bazuka_amd import lib as L
from oracle import pyref as pr
from util import synth_r1cs

pytestmark = pytest.mark.gpu

R = pr.R_MOD
_rnd = random.Random(424242)
TAU, ALPHA, BETA = (_rnd.randrange(1, R) for _ in range(3))
SECRETS = b"".join(pr.fr_to_mont_bytes(x) for x in (TAU, ALPHA, BETA))
SEED = bytes(range(32))


@pytest.mark.parametrize("log_m", [3, 8])
def test_contribution_and_check_equal_the_host_route(bzk, log_m):
    trivial = L.ptau_init(log_m)
    after, key = bzk.ptau_contribute(trivial, SECRETS)
    assert (after, key) == L.ptau_contribute(None, trivial, SECRETS)
    if log_m == 3:
        assert after == pc.oracle_accumulator(3, TAU, ALPHA, BETA) and key == pc.oracle_key(TAU, ALPHA, BETA)
    ok = (1, (0, 0, 0, 0))
    assert bzk.ptau_check(trivial, key, after, SEED) == ok == L.ptau_check(None, trivial, key, after, SEED)
    assert bzk.ptau_check(None, None, after, SEED) == ok
    m = 1 << log_m
    e = lambda name, i: pc.entry(after, log_m, name, i)
    forged = pc.with_entry(pc.with_entry(after, log_m, "alpha_g1", m - 2, e("alpha_g1", m - 1)), log_m, "alpha_g1", m - 1, e("alpha_g1", m - 2))
    got = bzk.ptau_check(trivial, key, forged, SEED)
    assert got == (0, (3, 0, 0, 0)) and got == L.ptau_check(None, trivial, key, forged, SEED)


def _csr_bytes(r1):
    out = []
    for which in range(3):
        rp, col, val = array.array("I", [0]), array.array("I"), []
        for row in r1["rows"]:
            for v, c in row[which]:
                col.append(v)
                val.append(pr.fr_to_mont_bytes(c))
            rp.append(len(col))
        out.append((len(r1["rows"]), rp.tobytes(), col.tobytes(), b"".join(val)))
    return out


def test_the_accumulator_holds_the_device_key_s_points(bzk, co):
    """log_m = 4: with delta = gamma = 1 the h query of bzk_groth16_setup is tau_g1[i + m] - tau_g1[i], and alpha_g1, beta_g1, beta_g2 of its head are
    entry 0 of their arrays"""
    r1 = synth_r1cs(6, n_in=3, seed=77)  # 6 rows + 3 inputs: a domain of 16
    toxic = SECRETS + pr.fr_to_mont_bytes(1) * 2
    ph, vk = bzk.groth16_setup(_csr_bytes(r1), r1["n_in"], r1["n_aux"], toxic)
    h = bzk.params_read(ph, 1)
    bzk.params_free(ph)
    m = len(h) // 96 + 1
    assert m == 16 and len(h) == 96 * 15
    acc, _ = bzk.ptau_contribute(L.ptau_init(4), SECRETS)
    e = lambda name, i: pc.entry(acc, 4, name, i)
    minus_one = pr.fr_to_canon_bytes(R - 1)
    for i in range(m - 1):
        neg = co.g1_mul(e("tau_g1", i) + b"\0", minus_one)
        assert co.g1_add(e("tau_g1", i + m) + b"\0", neg) == h[96 * i:96 * i + 96] + b"\0", i
    assert vk[:97] == e("alpha_g1", 0) + b"\0" and vk[97:194] == e("beta_g1", 0) + b"\0" and vk[194:387] == e("beta_g2", 0) + b"\0"
