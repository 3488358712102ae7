"""Batched Jubjub EdDSA verification on the device (bzk_jubjub_verify_batch / _dev, eddsa.hip jubjub_verify_kernel) against the host verifier and
oracle/pyref.py, the hash-then-verify chain on device buffers, and the withdraw builder's batched signature checks (bzk_mpn_set_device) against the
host builder.  The CPU run of the same per-signature code: tests/test_eddsa_cpu.py."""
import pytest
import torch

import eddsa_cases as E
import r1cs_scenarios as sc
from bazuka_amd import lib as L
from oracle import pyref as pr

pytestmark = pytest.mark.gpu
F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
ZIESHA = F(1)


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _verify_dev(bzk, pub, msg, sig):
    n = len(msg) // 32
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d = [_dev(x) for x in (pub, msg, sig)]
    torch.cuda.synchronize()
    bzk.jubjub_verify_batch_dev(d[0], d[1], d[2], n, ok)
    bzk.sync()
    return bytes(ok.cpu().numpy().tobytes())


def test_case_list(bzk):
    cases = E.case_list()
    assert {c[0] for c in cases} == set(E.CLASSES)
    want = bytes(c[4] for c in cases)
    got = bzk.jubjub_verify_batch(b"".join(c[1] for c in cases), b"".join(c[2] for c in cases), b"".join(c[3] for c in cases))
    assert got == want, [(i, c[0], got[i], c[4]) for i, c in enumerate(cases) if got[i] != c[4]]


def test_arguments(bzk):
    lib, b = L.load_library(), bytes(96)
    assert bzk.jubjub_verify_batch(b"", b"", b"") == b""
    assert lib.bzk_jubjub_verify_batch(bzk.h, None, b, b, 1, b) == -1 and lib.bzk_jubjub_verify_batch_dev(bzk.h, b, b, None, 1, b) == -1
    assert lib.bzk_jubjub_verify_batch_dev(bzk.h, None, None, None, 0, None) == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 100000])
def test_sizes_host_pointers_and_device_buffers(bzk, n):
    pub, msg, sig = E.bulk(n, 1000 + n)
    want = E.host_verdicts(pub, msg, sig)
    assert want.count(1) == (n + 1) // 2
    assert bzk.jubjub_verify_batch(pub, msg, sig) == want
    assert _verify_dev(bzk, pub, msg, sig) == want


def test_more_than_one_staging_chunk(bzk):
    """the host-pointer form stages 2^20 signatures at a time: a call that needs two chunks, the second one short"""
    pub, msg, sig = E.bulk(4096, 5)
    want = E.host_verdicts(pub, msg, sig)
    n = (1 << 20) + 100
    rep = n // 4096 + 1
    got = bzk.jubjub_verify_batch((pub * rep)[:64 * n], (msg * rep)[:32 * n], (sig * rep)[:96 * n])
    assert got == (want * rep)[:n]


def test_hash_then_verify_stays_on_the_device(bzk):
    """the arity-7 hash of an MpnTransaction's fields (bzk_poseidon_batch_dev) is the message of the verification that follows it on the same stream"""
    import random
    rnd = random.Random(11)
    n = 1024
    keys = [L.host_jubjub_keys(b"chain %d" % k) for k in range(8)]
    tuples, pubs, sigs, msgs = [], [], [], []
    for i in range(n):
        t = b"".join(F(rnd.randrange(pr.R_MOD)) for _ in range(7))
        key = keys[i % 8]
        m = L.host_poseidon(t)
        sig = L.host_jubjub_sign(key, m)
        if i % 3 == 1:  # signed over another transaction
            t = t[:32] + F(rnd.randrange(pr.R_MOD)) + t[64:]
            m = L.host_poseidon(t)
        tuples.append(t); pubs.append(key[:64]); sigs.append(sig); msgs.append(m)
    pub, sig = b"".join(pubs), b"".join(sigs)
    want = E.host_verdicts(pub, b"".join(msgs), sig)
    assert want == bytes(0 if i % 3 == 1 else 1 for i in range(n))
    d_in, d_pub, d_sig = _dev(b"".join(tuples)), _dev(pub), _dev(sig)
    d_msg = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bzk.poseidon_batch_dev(d_in, 7, n, d_msg)
    bzk.jubjub_verify_batch_dev(d_pub, d_msg, d_sig, n, ok)
    bzk.sync()
    assert bytes(ok.cpu().numpy().tobytes()) == want


# ---- the withdraw builder
def _world(n, dev):
    w = L.MpnWorld(15, 3)
    if dev is not None:
        w.set_device(dev)
    idx = [(i * 7919 + 3) % (4 ** 15) for i in range(n)]
    for i, a in enumerate(idx):
        w.add_account(a, b"acct%d" % i, ZIESHA, 10 ** 9)
    w.set_height(3)
    return w, idx


def _signed_withdraw(i, nonce, amount, fee, fingerprint):
    key = L.host_jubjub_keys(b"acct%d" % i)
    sig = L.host_jubjub_sign(key, L.host_poseidon(fingerprint + F(nonce)))
    return [key[:64], nonce, ZIESHA, amount, ZIESHA, fee, fingerprint, sig]


def _queue_with_three_bad(w, idx):
    for i in range(64):
        if i in (5, 31, 63):  # signed elsewhere, and badly: s off by one / R off the curve / signed over another fingerprint
            a = _signed_withdraw(i, 1, 10 + i, 1, F(900 + i))
            if i == 5:
                a[7] = a[7][:64] + F((U(a[7][64:]) + 1) % pr.R_MOD)
            elif i == 31:
                a[7] = F((U(a[7][:32]) + 1) % pr.R_MOD) + a[7][32:]
            else:
                a[6] = F(1)
            w.push_withdraw_signed(*a)
        elif i % 2:
            w.push_withdraw_signed(*_signed_withdraw(i, 1, 10 + i, 1, F(900 + i)))
        else:
            w.push_withdraw(idx[i], ZIESHA, 10 + i, ZIESHA, 1, F(900 + i))


def test_device_builder_checks_signatures_in_batches_with_the_host_builders_result(bzk):
    (host, idx), (dev, _) = _world(64, None), _world(64, bzk)
    _queue_with_three_bad(host, idx)
    _queue_with_three_bad(dev, idx)
    bzk.prof_enable(True)
    bzk.prof_reset()
    try:
        rd = dev.withdraw_synthesize(3, F(12))
        bzk.sync()
        launches, _ = bzk.prof_query("jubjub_verify")
    finally:
        bzk.prof_enable(False)
    rh = host.withdraw_synthesize(3, F(12))
    assert (rh.accepted, rh.rejected, rh.satisfied) == (61, 3, True)
    assert (rd.accepted, rd.rejected, rd.satisfied) == (61, 3, True)
    assert (rh.n_in, rh.n_aux, rh.n_constraints) == (rd.n_in, rd.n_aux, rd.n_constraints)
    for k in ("z", "az", "bz", "cz", "a_density", "b_density"):
        assert rh.view(k) == rd.view(k), k
    assert host.root() == dev.root()
    assert 1 <= launches < 64, launches  # batched, not one launch per transaction


def test_device_builder_makes_the_same_work_bytes_for_wallet_style_withdrawals(bzk):
    out = []
    for d in (None, bzk):
        w, idx = _world(64, d)
        for i in range(64):
            w.push_withdraw(idx[i], ZIESHA, 10 + i, ZIESHA, i % 3)
        out.append(w.make_work(1, sc.VKS, 12, log4_batches=(1, 3, 1)).encode())
    assert out[0] == out[1] and len(out[0]) > 64 * 96
