"""Batched Ed25519 key derivation and signing on the device (bzk_ed25519_keys_batch / _dev, bzk_ed25519_sign_batch / _dev, bzk_mpn_deposits_sign,
bzk_l1_txs_sign) against the ctx = NULL route of the same entry points, which tests/test_ed25519_sign_cpu.py pins on the OpenSSL / RFC 8032
fixture and on ed25519_cases.sign; the signatures then go through the device verifier and the wire-form admission entries."""
import pytest
import torch

import ed25519_cases as E
import ed25519_sign_cases as S
import l1_tx_cases as T
from bazuka_amd import lib as L

pytestmark = pytest.mark.gpu

CANARY = 32


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).cuda()


def _offsets(msgs):
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    return torch.tensor(off, dtype=torch.int64, device="cuda")


def _bytes(t):
    return bytes(t.cpu().numpy().tobytes())


def _sign_dev(bzk, keys, msgs):
    n = len(msgs)
    data = b"".join(msgs)
    sig = torch.full((n * 64 + CANARY,), 7, dtype=torch.uint8, device="cuda")
    dk, dm, doff = _dev(keys), _dev(data), _offsets(msgs)
    off_before = _bytes(doff)
    torch.cuda.synchronize()
    bzk.ed25519_sign_batch_dev(dk, dm, doff, n, sig)
    bzk.sync()
    assert _bytes(dk) == keys and _bytes(dm) == (data or b"\0") and _bytes(doff) == off_before  # the caller's buffers are left alone
    out = _bytes(sig)
    assert out[64 * n:] == b"\x07" * CANARY                                                       # and nothing past the output is touched
    return out[:64 * n]


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_sign_batch_three_routes_agree(bzk, n):
    keys, msgs = S.key_rows(n, 100 + n), S.messages(n, 200 + n)
    want = L.host_ed25519_sign_batch(keys, msgs)
    for i in range(0, n, 37):
        assert want[64 * i:64 * i + 64] == E.sign(keys[64 * i:64 * i + 32], msgs[i]), i
    assert bzk.ed25519_sign_batch(keys, msgs) == want
    assert _sign_dev(bzk, keys, msgs) == want


def test_sign_then_verify_roundtrip(bzk):
    n = 4096
    keys, msgs = S.key_rows(n, 300), S.messages(n, 301, fixed_len=40)
    assert len(set(msgs)) == n and len({keys[64 * i:64 * i + 64] for i in range(n)}) == n
    sig = bzk.ed25519_sign_batch(keys, msgs)
    pks = b"".join(keys[64 * i + 32:64 * i + 64] for i in range(n))
    assert bzk.ed25519_verify_batch(pks, msgs, sig) == b"\x01" * n
    flipped = [T.flip(m, 8 + i % 32, i % 8) for i, m in enumerate(msgs)]
    assert bzk.ed25519_verify_batch(pks, flipped, sig) == bytes(n)


def test_sign_round_crossing(bzk):
    n = L.ED25519_SIGN_ROUND + 65
    keys, msgs = S.key_rows(n, 400), S.messages(n, 401, fixed_len=16)
    want = L.host_ed25519_sign_batch(keys, msgs)
    for i in list(range(0, n, n // 24))[:24] + list(range(L.ED25519_SIGN_ROUND - 4, L.ED25519_SIGN_ROUND + 4)):  # 32 rows, the boundary's among them
        assert want[64 * i:64 * i + 64] == E.sign(keys[64 * i:64 * i + 32], msgs[i]), i
    got = bzk.ed25519_sign_batch(keys, msgs)
    assert got == want, [i for i in range(n) if got[64 * i:64 * i + 64] != want[64 * i:64 * i + 64]][:8]


def test_keys_batch_three_routes_agree(bzk):
    seeds = S.seeds(65)
    n = len(seeds)
    want = L.host_ed25519_keys_batch(seeds)
    for i in range(len(S.SEED_LENGTHS) + 1):
        secret = S.secret_of(seeds[i])
        assert want[64 * i:64 * i + 64] == secret + E.public_key(secret), len(seeds[i])
    assert bzk.ed25519_keys_batch(seeds) == want
    data, doff = _dev(b"".join(seeds)), _offsets(seeds)
    out = torch.full((n * 64 + CANARY,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bzk.ed25519_keys_batch_dev(data, doff, n, out)
    bzk.sync()
    assert _bytes(data) == b"".join(seeds) and _bytes(out) == want + b"\x07" * CANARY
    assert bzk.ed25519_keys_batch([]) == b"" and bzk.ed25519_sign_batch(b"", []) == b""


def test_deposits_sign_then_admit(bzk):
    n = 257
    keys = S.key_rows(n, 500)
    other = S.key_rows(1, 501)[32:64]
    spoiled = set(range(4, n, 5))
    recs = [S.unsigned_deposit(other if i in spoiled else keys[64 * i + 32:64 * i + 64], "m" * (i % 130), nonce=i,
                               sig=bytes(range(64)) if i % 3 == 0 else None) for i in range(n)]
    blob = b"".join(E.enc(r) for r in recs)
    want = L.host_mpn_deposits_sign(keys, blob, n)
    assert want[1] == bytes(0 if i in spoiled else 1 for i in range(n))
    for i in (0, 1, 128, 256):
        assert want[0][64 * i:64 * i + 64] == E.sign(keys[64 * i:64 * i + 32], E.unsigned_bytes(recs[i])), i
    got = bzk.mpn_deposits_sign(keys, blob, n)
    assert got == want
    verdict, _ = bzk.mpn_deposit_verify_batch(got[2], n, want_address=False)
    assert bytes(v & 1 for v in verdict) == want[1]
    assert bzk.mpn_deposits_sign(keys, blob, n, want_txs=False) == (want[0], want[1], None)
    with pytest.raises(L.BzkError, match="record 256"):
        bzk.mpn_deposits_sign(keys, blob[:-1], n)


@pytest.mark.parametrize("form", [T.FORM_TX, T.FORM_TX_AND_DELTA])
def test_l1_txs_sign_then_verify(bzk, form):
    n = 257
    keys = S.key_rows(n, 600)
    other = S.key_rows(1, 601)[32:64]
    txs = S.l1_mixed(n, [other if i % 11 == 10 else keys[64 * i + 32:64 * i + 64] for i in range(n)])
    blob = b"".join(T.enc(t, form, False, T.delta_pairs(i % 3) if form == T.FORM_TX_AND_DELTA and i % 2 else None) for i, t in enumerate(txs))
    want = L.host_l1_txs_sign(keys, blob, n, form)
    assert want[1] == bytes(0 if (i % 9 == 8 or i % 11 == 10) else 1 for i in range(n))
    for i in (0, 5, 6, 257 - 1):
        if want[1][i]:
            assert want[0][64 * i:64 * i + 64] == E.sign(keys[64 * i:64 * i + 32], T.signed_bytes(txs[i])), i
    got = bzk.l1_txs_sign(keys, blob, n, form)
    assert got == want
    ok, h = bzk.l1_tx_verify_batch(got[3], n, form)
    assert all(ok[i] == 1 for i in range(n) if want[1][i])
    assert h == want[2]
    assert bzk.l1_txs_sign(keys, blob, n, form, want_hash=False, want_txs=False) == (want[0], want[1], None, None)
