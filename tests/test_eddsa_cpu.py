"""Batched Jubjub EdDSA verification (bzk_jubjub_verify_batch, bazuka_amd/csrc/bzk_eddsa.cuh) on the CPU: the kernel's per-signature function runs
through tests/host/eddsa_check.hip with the bound assertions of the 29-bit field on (an assertion that fires aborts the process), and is compared with
the two oracles - oracle/pyref.py jj_verify and the product's one-at-a-time host verifier bzk_host_jubjub_verify.  Then the entries' argument checks
and the host withdraw builder with signatures it did not make itself (bzk_mpn_push_withdraw_signed).  The device run: tests/test_gpu_eddsa.py."""
import ctypes as C
import os

import pytest

import eddsa_cases as E
from bazuka_amd import lib as L
from oracle import pyref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
ZIESHA = F(1)
BZK_OK, BZK_E_ARG = 0, -1


@pytest.fixture(scope="module")
def harness(co):
    lib = C.CDLL(os.path.join(ROOT, "tests", "host", "_eddsa_check.so"))
    consts = co.poseidon_params(6)

    def run(pub: bytes, msg: bytes, sig: bytes) -> bytes:
        n = len(msg) // 32
        assert len(pub) == 64 * n and len(sig) == 96 * n
        ok = C.create_string_buffer(max(n, 1))
        assert lib.ec_verify_batch(pub, msg, sig, C.c_uint64(n), consts, len(consts) // 32, 8, 57, ok) == 0
        return ok.raw[:n]
    return run


def test_reference_vector(harness):
    """src/crypto/jubjub/mod.rs:183-193: keys from b"ABC", message 123456 verifies, 123457 does not"""
    key = L.host_jubjub_keys(b"ABC")
    sig = L.host_jubjub_sign(key, F(123456))
    assert harness(key[:64] * 2, F(123456) + F(123457), sig * 2) == b"\x01\x00"
    assert L.host_jubjub_verify(key[:64], F(123456), sig) and not L.host_jubjub_verify(key[:64], F(123457), sig)


def test_case_list_against_pyref_and_the_host_verifier(harness):
    cases = E.case_list()
    assert {c[0] for c in cases} == set(E.CLASSES)
    want = bytes(c[4] for c in cases)
    assert set(want) == {0, 1}
    by_class = {k: [c[4] for c in cases if c[0] == k] for k in E.CLASSES}
    assert by_class["valid"] == [1] * 8 and by_class["s + ORDER"] == [1, 1] and by_class["pk = (0, 1)"] == [1]
    assert by_class["pk = (0, -1)"] == [1] * 4 and by_class["non-canonical"] == [0] * 8
    for k in ("msg", "s", "r.x", "pk.x", "pk.y"):
        assert by_class[k] == [0] * 8, k
    # at least three of the order-2 cases only verify with h as the full integer: h mod ORDER has the other parity
    other = 0
    for cls, pub, msg, sig, _ in cases:
        if cls == "pk = (0, -1)":
            h = pr.poseidon([U(sig[:32]), U(sig[32:64]), U(pub[:32]), U(pub[32:]), U(msg)])
            other += (h % pr.JJ_ORDER) % 2 != h % 2
    assert other >= 3
    got = harness(b"".join(c[1] for c in cases), b"".join(c[2] for c in cases), b"".join(c[3] for c in cases))
    assert got == want, [(i, c[0], got[i], c[4]) for i, c in enumerate(cases) if got[i] != c[4]]
    for cls, pub, msg, sig, verdict in cases:
        if cls != "non-canonical":
            assert L.host_jubjub_verify(pub, msg, sig) == bool(verdict), cls


def test_volume_against_the_host_verifier(harness):
    pub, msg, sig = E.bulk(2000, 7)
    want = E.host_verdicts(pub, msg, sig)
    assert want[0::2] == b"\x01" * 1000 and want[1::2] == b"\x00" * 1000
    assert harness(pub, msg, sig) == want


def test_entries_refuse_bad_arguments_without_touching_a_device():
    lib = L.load_library()
    b = C.create_string_buffer(96)
    fake = C.create_string_buffer(4096)  # stands for a context: both entries return before they look into it
    for fn in (lib.bzk_jubjub_verify_batch, lib.bzk_jubjub_verify_batch_dev):
        assert fn(None, b, b, b, 1, b) == BZK_E_ARG
        assert fn(None, b, b, b, 0, b) == BZK_E_ARG
        for k in range(4):
            args = [b, b, b, b]
            args[k] = None
            assert fn(fake, args[0], args[1], args[2], 1, args[3]) == BZK_E_ARG, k
        assert fn(fake, None, None, None, 0, None) == BZK_OK  # n = 0: a no-op
    assert lib.bzk_mpn_push_withdraw_signed(None, b, 1, b, 1, b, 1, b, b) == BZK_E_ARG


# ---- the host builder with signatures made elsewhere
def _world(n_acc=10):
    w = L.MpnWorld(3, 3)
    for i in range(n_acc):
        w.add_account(i, b"acct%d" % i, ZIESHA, 10 ** 12)
    return w


def _signed_withdraw(i, nonce, amount, fee, fingerprint):
    key = L.host_jubjub_keys(b"acct%d" % i)
    sig = L.host_jubjub_sign(key, L.host_poseidon(fingerprint + F(nonce)))
    return key[:64], nonce, ZIESHA, amount, ZIESHA, fee, fingerprint, sig


def _same_arrays(a, b):
    assert (a.n_in, a.n_aux, a.n_constraints) == (b.n_in, b.n_aux, b.n_constraints)
    for k in ("z", "az", "bz", "cz", "a_density", "b_density"):
        assert a.view(k) == b.view(k), k


def test_host_builder_rejects_foreign_bad_signatures_and_nothing_else_moves():
    good = [_signed_withdraw(i, 1, 100 + i, i % 3, F(5000 + i)) for i in range(5)] + [_signed_withdraw(0, 2, 7, 1, F(6000))]
    b1 = list(_signed_withdraw(7, 1, 50, 1, F(7000)))
    b1[7] = b1[7][:64] + F((U(b1[7][64:]) + 1) % pr.R_MOD)                   # broken s
    b2 = list(_signed_withdraw(8, 1, 60, 1, F(8000)))
    b2[7] = F((U(b2[7][:32]) + 1) % pr.R_MOD) + b2[7][32:]                   # R off the curve
    clean, dirty = _world(), _world()
    for k, g in enumerate(good):
        clean.push_withdraw_signed(*g)
        if k == 2:
            dirty.push_withdraw_signed(*b1)
        dirty.push_withdraw_signed(*g)
    dirty.push_withdraw_signed(*b2)
    rc, rd = clean.withdraw_synthesize(2, F(8)), dirty.withdraw_synthesize(2, F(8))
    assert (rc.accepted, rc.rejected, rc.satisfied) == (6, 0, True)
    assert (rd.accepted, rd.rejected, rd.satisfied) == (6, 2, True)
    _same_arrays(rc, rd)
    assert clean.root() == dirty.root()


def test_push_withdraw_signed_equals_push_withdraw_with_that_fingerprint():
    a, b = _world(3), _world(3)
    a.push_withdraw(1, ZIESHA, 400, ZIESHA, 2, F(4242))
    b.push_withdraw_signed(*_signed_withdraw(1, 1, 400, 2, F(4242)))
    ra, rb = a.withdraw_synthesize(1, F(3)), b.withdraw_synthesize(1, F(3))
    assert (ra.accepted, ra.rejected, ra.satisfied) == (rb.accepted, rb.rejected, rb.satisfied) == (1, 0, True)
    _same_arrays(ra, rb)
