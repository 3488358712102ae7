"""The wire-form withdrawal producer on the device (bzk_mpn_withdraws_sign: mpn_withdraw_sign_kernel behind the SHA3 launch) against the records
oracle/pyref.py signs (tests/withdraw_sign_cases.py) and against the ctx = NULL route of the same entry, which tests/test_withdraw_sign_cpu.py
pins on pyref; the records then go through the device verifier and device admission."""
import pytest

import r1cs_scenarios as sc
import withdraw_cases as W
import withdraw_sign_cases as K
from bazuka_amd import lib as L

pytestmark = pytest.mark.gpu


def _draw(pairs, n):
    """n rows drawn in turn from [(record, key)]: (keys, blob, the encoded records)"""
    encs = [W.enc(r) for r, _ in pairs]
    return b"".join(pairs[i % len(pairs)][1] for i in range(n)), b"".join(encs[i % len(pairs)] for i in range(n)), encs


def _split(blob, lens):
    out, at = [], 0
    for k in lens:
        out.append(blob[at:at + k])
        at += k
    assert at == len(blob)
    return out


def test_fixed_list_and_refusals_equal_pyref(bzk):
    good = K.fixed()
    refused = [(rec, key) for _, rec, key in K.refusals()]
    rows = []
    for i, g in enumerate(good):                                                               # a refusal between every two signed records
        rows += [g, refused[i]]
    rows.append(refused[9])
    keys, blob, n = K.batch(rows)
    out, ok, fp = bzk.mpn_withdraws_sign(keys, blob, n)
    assert ok == bytes(1 if len(r) == 3 else 0 for r in rows)
    assert fp == b"".join(W.F(W.fingerprint(r[0])) for r in rows)
    assert out == b"".join(W.enc(r[2] if len(r) == 3 else r[0]) for r in rows)
    assert bzk.mpn_withdraws_sign(keys, blob, n, want_fingerprint=False) == (out, ok, None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_mixed_lengths_equal_the_host_route(bzk, n):
    pairs = K.pool(8, 31, memo_base=1, spoil=True)
    assert len({len(W.enc(r)) % 8 for r, _ in pairs}) == 8                                     # record and payment offsets take every alignment
    keys, blob, _ = _draw(pairs, n)
    want = L.host_mpn_withdraws_sign(keys, blob, n)
    assert want[1] == bytes(0 if i % 8 == 7 else 1 for i in range(n))
    assert bzk.mpn_withdraws_sign(keys, blob, n) == want


def test_the_output_verifies_on_the_device(bzk):
    n = 257
    pairs = K.pool(8, 32, memo_base=1)
    keys, blob, encs = _draw(pairs, n)
    out, ok, fp = bzk.mpn_withdraws_sign(keys, blob, n)
    assert ok == b"\x01" * n
    assert bzk.mpn_withdraw_verify_batch(out, n) == (b"\x03" * n, fp)
    flipped, at = bytearray(out), 0
    for i in range(n):
        flipped[at + 133 + 8] ^= 1                                                             # the first memo byte: the signature breaks, the calldata stands
        at += len(encs[i % 8])
    assert bzk.mpn_withdraw_verify_batch(bytes(flipped), n)[0] == b"\x02" * n


def test_round_crossing_at_the_record_limit(bzk):
    n = L.MPN_TX_CHUNK + 65
    pairs = K.pool(8, 33)
    spoiled = [(r, k[:96] + K.D.R_LIMBS) for r, k in pairs]
    want = L.host_mpn_withdraws_sign(*K.batch(pairs))
    want_bad = L.host_mpn_withdraws_sign(*K.batch(spoiled))
    assert want[1] == b"\x01" * 8 and want_bad[1] == bytes(8)
    lens = [len(W.enc(r)) for r, _ in pairs]
    assert len(set(lens)) == 8
    rec_ok, rec_bad = _split(want[0], lens), _split(want_bad[0], lens)
    bad = [i % 5 == 4 for i in range(n)]
    keys = b"".join((spoiled if bad[i] else pairs)[i % 8][1] for i in range(n))
    blob = b"".join(W.enc(pairs[k][0]) for k in range(8))
    blob = b"".join(_split(blob, lens)[i % 8] for i in range(n))
    out, ok, fp = bzk.mpn_withdraws_sign(keys, blob, n)
    assert ok == bytes(0 if b else 1 for b in bad)
    assert fp == b"".join(want[2][32 * (i % 8):32 * (i % 8) + 32] for i in range(n))
    assert out == b"".join((rec_bad if bad[i] else rec_ok)[i % 8] for i in range(n))


def test_round_crossing_at_the_byte_limit(bzk):
    n = 1030
    pairs = [(K.unsigned(b"wd sign big %d" % k, 5 + k, "B" * (65388 - 3 * k), W.ZIESHA, W.ZIESHA, 77 + k, W.ZIESHA, k), K.key_of(b"wd sign big %d" % k))
             for k in range(2)]
    lens = [len(W.enc(r)) for r, _ in pairs]
    assert lens == [133 + 65500, 133 + 65497] and 515 * (65500 + 65497) > L.MPN_WD_CHUNK_BYTES and n < L.MPN_TX_CHUNK
    want = L.host_mpn_withdraws_sign(*K.batch(pairs))
    assert want[1] == b"\x01\x01"
    recs = _split(want[0], lens)
    keys, blob, _ = _draw(pairs, n)
    out, ok, fp = bzk.mpn_withdraws_sign(keys, blob, n)
    assert ok == b"\x01" * n
    assert fp == want[2] * (n // 2)
    assert out == b"".join(recs[i % 2] for i in range(n))


def test_device_admission_of_the_produced_records(bzk):
    want_blob, want_root, good = W.world_a()
    keys = b"".join(K.key_of(b"acct%d" % acct) for acct, _, _ in W.WITHDRAWALS)
    blank = b"".join(W.enc(K.blanked(r, K.JUNK[i % 2])) for i, r in enumerate(good))
    out, ok, _ = bzk.mpn_withdraws_sign(keys, blank, len(good))
    assert ok == b"\x01" * len(good) and out == b"".join(W.enc(r) for r in good)
    dev = W.admission_world(bzk)
    assert dev.push_withdraws(out, len(good)) == (b"\x01" * len(good), len(good))
    assert dev.make_work(1, sc.VKS, 10, log4_batches=(1, 2, 1)).encode() == want_blob and dev.root() == want_root


def test_arguments(bzk):
    lib = L.load_library()
    rows = K.fixed()[:3]
    keys, blob, n = K.batch(rows)
    assert lib.bzk_mpn_withdraws_sign(bzk.h, None, None, 0, 0, None, None, None) == 0
    assert bzk.mpn_withdraws_sign(b"", b"", 0) == (b"", b"", b"")
    with pytest.raises(L.BzkError, match="record 2"):
        bzk.mpn_withdraws_sign(keys, blob[:-1], n)
    want = b"".join(W.enc(r[2]) for r in rows)
    assert bzk.mpn_withdraws_sign(keys, blob, n, want_fingerprint=False) == (want, b"\x01" * n, None)    # NULL fingerprint_out
    assert lib.bzk_mpn_withdraws_sign(bzk.h, keys, blob, len(blob), n, None, keys, None) == -1
