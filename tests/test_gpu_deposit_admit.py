"""Device SHA-512, Ed25519 and wire-form deposit admission on the GPU (bzk_sha512_batch / _dev, bzk_ed25519_verify_batch / _dev,
bzk_mpn_deposit_verify_batch, bzk_mpn_push_deposits with bzk_mpn_set_device) against hashlib, the restatement tests/ed25519_cases.py and the
ctx = NULL path, which tests/test_ed25519_cpu.py and tests/test_deposit_admit_cpu.py pin.  No build of the library lowers the chunk size of the
withdrawal or the deposit path, so a batch that crosses a chunk end (2^16 records) is not part of this file: it would take minutes of Python
signing or a 2^16-record copy of few records, which tools/deposit_admit_bench.py runs instead (its 2^18 row, checked against the host path)."""
import copy
import hashlib
import random

import pytest
import torch

import decompress_cases as Dc
import ed25519_cases as E
import r1cs_scenarios as sc
import withdraw_cases as Wd
from bazuka_amd import lib as L

pytestmark = pytest.mark.gpu
SIZES = [1, 64, 65, 300]


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _offsets(msgs):
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    return _dev(b"".join(msgs) + b"\0"), torch.tensor(off, dtype=torch.int64).cuda()


@pytest.mark.parametrize("n", SIZES)
def test_sha512_mixed_lengths_in_one_batch(bzk, n):
    """lengths 0 .. 300 mixed, so the lanes of a wave leave the block loop after one, two and three trips"""
    msgs = E.messages([(97 * i + n) % 301 for i in range(n)], 5000 + n)
    want = b"".join(hashlib.sha512(m).digest() for m in msgs)
    assert bzk.sha512_batch(msgs) == want
    data, off = _offsets(msgs)
    dig = torch.full((n * 64,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bzk.sha512_batch_dev(data, off, n, dig)
    bzk.sync()
    assert bytes(dig.cpu().numpy().tobytes()) == want


def test_sha512_every_length_to_300(bzk):
    msgs = E.messages(list(range(301)), 12)
    assert bzk.sha512_batch(msgs) == b"".join(hashlib.sha512(m).digest() for m in msgs)
    assert bzk.sha512_batch([]) == b""


_cases = None


def signature_cases():
    """[(pk, msg, sig, verdict by the restatement)]: the golden triples with every fourth one corrupted, then the edge cases of the recalled
    rules.  Built once."""
    global _cases
    if _cases is None:
        rnd = random.Random(61)
        out = []
        for i, (pk, msg, sig) in enumerate(E.golden_vectors()):
            if i % 4 == 3:
                variants = E.corrupted(pk, msg, sig, rnd)
                pk, msg, sig = variants[(i // 4) % len(variants)][1:]
            out.append((pk, msg, sig))
        pk, msg, sig = E.golden_vectors()[4]
        out.append((pk, msg, sig[:32] + (int.from_bytes(sig[32:], "little") + E.L_ORDER).to_bytes(32, "little")))   # s + l
        key, forged = E.small_order_forgery(b"small order")
        out.append((key, b"small order", forged))
        for key in E.IDENTITY_KEYS.values():                                                                         # x = 0 with the sign bit; y = p + 1
            out.append((key, b"any", E.identity_key_forgery()))
        out.append((E.non_residue_y(), b"any", E.identity_key_forgery()))                                            # no root
        out.append((E.IDENTITY_KEYS["canonical"], b"r", (1).to_bytes(32, "little") + bytes(32)))                     # R = (0, 1), canonical
        out.append((E.IDENTITY_KEYS["canonical"], b"r", (E.P + 1).to_bytes(32, "little") + bytes(32)))               # the same point, y = p + 1
        _cases = [c + (1 if E.verify(*c) else 0,) for c in out]
        assert [c[3] for c in _cases[-9:]] == [0, 1, 1, 1, 1, 1, 0, 1, 0]
    return _cases


@pytest.mark.parametrize("n", SIZES)
def test_ed25519_against_the_restatement(bzk, n):
    cases = signature_cases()
    start = 0 if n > 1 else len(cases) - 8  # n = 1: the small-order forgery
    batch = [cases[(start + i) % len(cases)] for i in range(n)]
    want = bytes(c[3] for c in batch)
    pks, msgs, sigs = b"".join(c[0] for c in batch), [c[1] for c in batch], b"".join(c[2] for c in batch)
    assert bzk.ed25519_verify_batch(pks, msgs, sigs) == want
    assert L.host_ed25519_verify_batch(pks, msgs, sigs) == want
    data, off = _offsets(msgs)
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    dpk, dsig = _dev(pks), _dev(sigs)
    torch.cuda.synchronize()
    bzk.ed25519_verify_batch_dev(dpk, data, off, dsig, n, ok)
    bzk.sync()
    assert bytes(ok.cpu().numpy().tobytes()) == want


def test_arguments(bzk):
    lib, b = L.load_library(), bytes(128)
    off = (L.C.c_uint64 * 2)(0, 3)
    bad = (L.C.c_uint64 * 3)(0, 5, 3)
    assert lib.bzk_sha512_batch(bzk.h, None, None, 0, None) == 0 and lib.bzk_sha512_batch_dev(bzk.h, None, None, 0, None) == 0
    assert lib.bzk_sha512_batch(bzk.h, b, off, 1, None) == -1 and lib.bzk_sha512_batch(bzk.h, b, bad, 2, b) == -1
    assert lib.bzk_sha512_batch_dev(None, b, off, 1, b) == -1
    assert lib.bzk_ed25519_verify_batch(bzk.h, None, None, None, None, 0, None) == 0
    assert lib.bzk_ed25519_verify_batch(bzk.h, b, b, off, None, 1, b) == -1 and lib.bzk_ed25519_verify_batch(bzk.h, b, b, bad, b, 2, b) == -1
    assert lib.bzk_ed25519_verify_batch_dev(None, b, b, off, b, 1, b) == -1


def deposit_pool():
    """signed deposits over the memo lengths at SHA-512's edges and a few others, each with its variants: as signed (3), amount changed (2), an
    address without a root (1), both (0), no signature (2)"""
    rnd = random.Random(62)
    out = []
    for k, ml in enumerate((0, 9, 58, 59, 74, 75, 76, 200, 1000)):
        r = E.signed_deposit(b"pool %d" % k, E.account_address(k % E.N_ACC), "p" * ml, E.custom(E.MPN_CONTRACT) if k % 2 else E.ZIESHA, E.ZIESHA,
                             100 + k, E.ZIESHA, k)
        bad_sig, bad_key, unsigned = copy.deepcopy(r), copy.deepcopy(r), copy.deepcopy(r)
        bad_sig["payment"]["amount"]["amount"] += 1
        bad_key["mpn_address"]["x"] = Dc.no_root_x(rnd)
        both = copy.deepcopy(bad_sig)
        both["mpn_address"]["x"] = Dc.R_LIMBS
        unsigned["payment"]["sig"] = None
        out.append([E.enc(x) for x in (r, bad_sig, bad_key, both, unsigned)])
    return out


@pytest.mark.parametrize("n", SIZES)
def test_deposit_verdicts_and_addresses_equal_the_host_path(bzk, n):
    pool = deposit_pool()
    rnd = random.Random(63 + n)
    recs = [pool[rnd.randrange(len(pool))][i % 5] for i in range(n)]
    blob = b"".join(recs)
    want = L.host_mpn_deposit_verify_batch(blob, n)
    if n >= 64:
        assert {0, 1, 2, 3} <= set(want[0])  # agreement is not vacuous
    else:
        assert want[0] == b"\x03"
    got = bzk.mpn_deposit_verify_batch(blob, n)
    assert got[0] == want[0], [i for i in range(n) if got[0][i] != want[0][i]][:10]
    assert got[1] == want[1]
    assert bzk.mpn_deposit_verify_batch(blob, n, want_address=False) == (want[0], None)
    with pytest.raises(L.BzkError, match="record"):
        bzk.mpn_deposit_verify_batch(blob[:-1], n)


def test_device_admission_queues_what_the_host_path_queues(bzk):
    records = E.admission_records()
    bad_sig = copy.deepcopy(records[1])
    bad_sig["payment"]["nonce"] += 1
    wrong_id = E.signed_deposit(b"w1", E.account_address(1), "", E.custom(E.MPN_CONTRACT + 1), E.ZIESHA, 5)
    mixed = records[:2] + [bad_sig] + records[2:4] + [wrong_id] + records[4:]
    blob = b"".join(E.enc(r) for r in mixed)
    host, dev = Wd.admission_world(), Wd.admission_world(bzk)
    bzk.prof_enable(True)
    bzk.prof_reset()
    try:
        got_dev = dev.push_deposits(blob, len(mixed))
        bzk.sync()
        launches = {k: bzk.prof_query(k)[0] for k in ("ed25519_verify", "jubjub_decompress", "mpn_deposit_verdict")}
    finally:
        bzk.prof_enable(False)
    assert launches == {"ed25519_verify": 1, "jubjub_decompress": 1, "mpn_deposit_verdict": 1}
    assert got_dev == host.push_deposits(blob, len(mixed)) == (bytes([1, 1, 0, 1, 1, 0, 1]), len(records))
    wd, wh = (w.make_work(0, sc.VKS, 10, log4_batches=(2, 1, 1)).encode() for w in (dev, host))
    assert wd == wh and dev.root() == host.root()
