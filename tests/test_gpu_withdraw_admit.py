"""Device SHA3-256 and wire-form withdrawal admission on the GPU (bzk_sha3_256_batch / _dev, bzk_mpn_withdraw_verify_batch, bzk_mpn_push_withdraws
with bzk_mpn_set_device) against hashlib and the product's host path, which tests/test_withdraw_admit_cpu.py pins on the independent Python route
of tests/withdraw_cases.py.  The CPU run of the same per-lane code is in that file."""
import hashlib

import pytest
import torch

import r1cs_scenarios as sc
import withdraw_cases as Wd
from bazuka_amd import lib as L
from bazuka_amd import worker as W
from util import fr_bytes, fr_list

pytestmark = pytest.mark.gpu
ALICE = bytes(range(1, 33))


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _sha3_dev(bzk, msgs):
    n = len(msgs)
    off = [0]
    for m in msgs:
        off.append(off[-1] + len(m))
    data, doff = _dev(b"".join(msgs) + b"\0"), torch.tensor(off, dtype=torch.int64).cuda()
    dig = torch.full((n * 32,), 7, dtype=torch.uint8, device="cuda")
    sc = torch.full((n * 32,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bzk.sha3_256_batch_dev(data, doff, n, dig, sc)
    bzk.sync()
    return bytes(dig.cpu().numpy().tobytes()), bytes(sc.cpu().numpy().tobytes())


def _want(msgs):
    digs = [hashlib.sha3_256(m).digest() for m in msgs]
    return b"".join(digs), b"".join(L.host_scalar_new(d) for d in digs)


def test_sha3_every_length_to_300_and_one_long_message_in_one_call(bzk):
    msgs = Wd.messages(list(range(301)) + [65536], 11)
    want = _want(msgs)
    assert want[1] == b"".join(Wd.scalar_new(want[0][32 * i:32 * i + 32]) for i in range(len(msgs)))
    assert bzk.sha3_256_batch(msgs) == want
    assert _sha3_dev(bzk, msgs) == want
    assert bzk.sha3_256_batch(msgs, want_scalar=False) == (want[0], None) and bzk.sha3_256_batch(msgs, want_digest=False) == (None, want[1])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_sha3_sizes_of_mixed_lengths(bzk, n):
    msgs = Wd.messages([(37 * i + n) % 420 for i in range(n)], 3000 + n)
    want = _want(msgs)
    assert bzk.sha3_256_batch(msgs) == want
    assert _sha3_dev(bzk, msgs) == want


def test_sha3_host_form_across_both_limits_of_a_staging_chunk(bzk):
    """the host form stages 2^20 messages or 64 MiB per round: 70 messages of 1 MiB need two rounds by bytes, 2^20 + 5 short ones two by count"""
    big = Wd.messages([1 << 20], 7)[0]
    msgs = [big[k:] + big[:k] for k in range(70)]
    assert bzk.sha3_256_batch(msgs, want_scalar=False)[0] == b"".join(hashlib.sha3_256(m).digest() for m in msgs)
    short = [b"", b"a", b"ab"]
    n = (1 << 20) + 5
    digs = [hashlib.sha3_256(m).digest() for m in short]
    got = bzk.sha3_256_batch([short[i % 3] for i in range(n)], want_scalar=False)[0]
    assert got == (b"".join(digs) * (n // 3 + 1))[:32 * n]


def test_sha3_arguments(bzk):
    lib, b = L.load_library(), bytes(96)
    off = (L.C.c_uint64 * 2)(0, 3)
    assert bzk.sha3_256_batch([]) == (b"", b"")
    for fn in (lib.bzk_sha3_256_batch, lib.bzk_sha3_256_batch_dev):
        assert fn(bzk.h, None, None, 0, None, None) == 0 and fn(None, b, off, 1, b, b) == -1
        assert fn(bzk.h, None, off, 1, b, b) == -1 and fn(bzk.h, b, None, 1, b, b) == -1
        assert fn(bzk.h, b, off, 1, None, None) == -1  # both outputs NULL
    bad = (L.C.c_uint64 * 3)(0, 5, 3)
    assert lib.bzk_sha3_256_batch(bzk.h, b, bad, 2, b, b) == -1  # decreasing offsets
    bad0 = (L.C.c_uint64 * 2)(1, 3)
    assert lib.bzk_sha3_256_batch(bzk.h, b, bad0, 1, b, b) == -1  # off[0] != 0


def test_withdraw_fixed_list(bzk):
    cases = Wd.fixed_list()
    blob = b"".join(Wd.enc(c[1]) for c in cases)
    want = (bytes(c[2] for c in cases), b"".join(c[3] for c in cases))
    assert L.host_mpn_withdraw_verify_batch(blob, len(cases)) == want
    got = bzk.mpn_withdraw_verify_batch(blob, len(cases))
    assert got[0] == want[0], [(i, c[0], got[0][i], c[2]) for i, c in enumerate(cases) if got[0][i] != c[2]]
    assert got[1] == want[1]
    assert bzk.mpn_withdraw_verify_batch(blob, len(cases), want_fingerprint=False) == (want[0], None)
    with pytest.raises(L.BzkError, match="record"):
        bzk.mpn_withdraw_verify_batch(blob[:-1], len(cases))
    lib = L.load_library()
    assert lib.bzk_mpn_withdraw_verify_batch(bzk.h, None, 0, 0, None, None) == 0 and lib.bzk_mpn_withdraw_verify_batch(bzk.h, None, 0, 1, blob, None) == -1


def test_withdraw_scalars_that_are_not_residues(bzk):
    rec, bad = Wd.non_residue_variants()
    blob = Wd.enc(rec) + b"".join(Wd.enc(r) for r in bad)
    want = L.host_mpn_withdraw_verify_batch(blob, 1 + len(bad))
    assert want[0] == b"\x03" + bytes(len(bad))
    assert bzk.mpn_withdraw_verify_batch(blob, 1 + len(bad)) == want


def _bulk_equals_host(bzk, recs):
    n, blob = len(recs), b"".join(recs)
    want = L.host_mpn_withdraw_verify_batch(blob, n)
    assert {0, 1, 2, 3} <= set(want[0])  # agreement is not vacuous
    got = bzk.mpn_withdraw_verify_batch(blob, n)
    assert got[0] == want[0], [i for i in range(n) if got[0][i] != want[0][i]][:10]
    assert got[1] == want[1]


def test_withdraw_bulk_across_the_record_limit_of_a_chunk(bzk):
    """a chunk ends at 2^16 records: 70 000 records with empty memos need two, the second one short"""
    recs = Wd.bulk(70000, 41)
    assert {len(r) for r in recs} == {245 + 32}  # a Custom contract id
    _bulk_equals_host(bzk, recs)


def test_withdraw_bulk_across_the_byte_limit_of_a_chunk(bzk):
    """a chunk ends at 64 MiB of payment bytes: 1 150 payments of 60 144 bytes are 66.0 MiB"""
    recs = Wd.bulk(1150, 43, memo_len=60000, pool=8)
    assert sum(len(r) - 133 for r in recs) > (64 << 20) and len(recs) < (1 << 16)
    _bulk_equals_host(bzk, recs)


def test_device_admission_makes_the_same_work_and_its_proof_verifies(bzk):
    want_blob, want_root, good = Wd.world_a()
    bad = Wd.bad_withdrawals(good)
    mixed = good[:1] + [bad[0][1]] + good[1:3] + [bad[1][1], bad[2][1]] + good[3:] + [bad[3][1]]
    host, dev = Wd.admission_world(), Wd.admission_world(bzk)
    bzk.prof_enable(True)
    bzk.prof_reset()
    try:
        got_dev = Wd.admit(dev, mixed)
        bzk.sync()
        launches = {k: bzk.prof_query(k)[0] for k in ("jubjub_decompress", "jubjub_verify", "sha3_256")}
    finally:
        bzk.prof_enable(False)
    assert launches == {"jubjub_decompress": 1, "jubjub_verify": 1, "sha3_256": 1}
    assert got_dev == Wd.admit(host, mixed) == (bytes(0 if any(r is b for _, b in bad) else 1 for r in mixed), len(good))
    wd = dev.make_work(1, sc.VKS, 10, log4_batches=(1, 2, 1)).encode()
    assert wd == host.make_work(1, sc.VKS, 10, log4_batches=(1, 2, 1)).encode() == want_blob
    assert dev.root() == host.root() == want_root
    # one Withdraw proof over a work admitted on the device, in the small shape the worker tests prove
    keys = W.DevSetup(bzk, {k: fr_bytes(fr_list(5, 9000 + k)) for k in range(3)})
    try:
        vks = [keys.keys(k, 3, 3, 1)[1] for k in range(3)]
        small = Wd.admission_world(bzk)
        assert Wd.admit(small, [good[0], bad[0][1], good[1], good[2]]) == (b"\x01\x00\x01\x01", 3)
        blob = small.make_work(1, vks, 300).encode()
        worker = W.Worker(bzk, ALICE, ("127.0.0.1", 9), keys)
        work = L.MpnWork.decode(blob)
        proof = worker.prove(work)
        assert proof is not None and len(proof) == 387 and work.verify(ALICE, proof)
    finally:
        keys.close()
