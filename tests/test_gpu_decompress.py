"""Key decompression, signature checks on compressed keys and wire-form transaction admission on the device (bzk_jubjub_decompress_batch / _dev,
bzk_jubjub_verify_batch_compressed, bzk_mpn_tx_verify_batch, bzk_mpn_push_txs with bzk_mpn_set_device) against the product's host mirror and host
path, which tests/test_decompress_cpu.py pins on oracle/pyref.py and oracle/pycircuit.py.  The CPU run of the same per-lane code is in that file."""
import pytest
import torch

import decompress_cases as D
import eddsa_cases as E
import r1cs_scenarios as sc
from bazuka_amd import lib as L
from bazuka_amd import worker as W
from util import fr_bytes, fr_list

pytestmark = pytest.mark.gpu
ALICE = bytes(range(1, 33))


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _decompress_dev(bzk, x, odd):
    n = len(odd)
    xy = torch.full((n * 64,), 7, dtype=torch.uint8, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    dx, dodd = _dev(x), _dev(odd)
    torch.cuda.synchronize()
    bzk.jubjub_decompress_batch_dev(dx, dodd, n, xy, ok)
    bzk.sync()
    return bytes(xy.cpu().numpy().tobytes()), bytes(ok.cpu().numpy().tobytes())


def test_fixed_keys(bzk):
    cases = D.fixed_keys()
    x, odd = b"".join(c[1] for c in cases), bytes(c[2] for c in cases)
    want = D.host_decompress_all(x, odd)
    assert want == (b"".join(D.expect(c[1], c[2])[0] for c in cases), bytes(D.expect(c[1], c[2])[1] for c in cases))
    assert set(want[1]) == {0, 1}
    got = bzk.jubjub_decompress_batch(x, odd)
    assert got == want, [(i, c[0]) for i, c in enumerate(cases) if got[1][i] != want[1][i] or got[0][64 * i:64 * i + 64] != want[0][64 * i:64 * i + 64]]
    assert _decompress_dev(bzk, x, odd) == want


def test_arguments(bzk):
    lib, b = L.load_library(), bytes(96)
    assert bzk.jubjub_decompress_batch(b"", b"") == (b"", b"")
    assert bzk.jubjub_verify_batch_compressed(b"", b"", b"", b"") == b""
    for fn in (lib.bzk_jubjub_decompress_batch, lib.bzk_jubjub_decompress_batch_dev):
        assert fn(bzk.h, None, None, 0, None, None) == 0 and fn(None, b, b, 1, b, b) == -1
        for k in range(4):
            args = [b, b, b, b]
            args[k] = None
            assert fn(bzk.h, args[0], args[1], 1, args[2], args[3]) == -1, k
    for fn in (lib.bzk_jubjub_verify_batch_compressed, lib.bzk_jubjub_verify_batch_compressed_dev):
        assert fn(bzk.h, None, None, None, None, 0, None) == 0 and fn(None, b, b, b, b, 1, b) == -1
        for k in range(5):
            args = [b, b, b, b, b]
            args[k] = None
            assert fn(bzk.h, args[0], args[1], args[2], args[3], 1, args[4]) == -1, k
    assert lib.bzk_mpn_tx_verify_batch(bzk.h, None, 0, 0, None, None) == 0 and lib.bzk_mpn_tx_verify_batch(bzk.h, None, 0, 1, b, None) == -1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 100000])
def test_sizes_host_pointers_and_device_buffers(bzk, n):
    x, odd = D.bulk_keys(n, 2000 + n)
    want = D.host_decompress_all(x, odd)
    if n >= 4096:
        assert 0.4 * n < sum(want[1]) < 0.6 * n
    assert bzk.jubjub_decompress_batch(x, odd) == want
    assert _decompress_dev(bzk, x, odd) == want


def test_verify_on_compressed_keys_equals_verify_on_decompressed_keys(bzk):
    pub, msg, sig = E.bulk(4096, 21)
    n = 4096
    keys = [D.compress(pub[64 * i:64 * i + 64]) for i in range(n)]
    x, odd = b"".join(k[0] for k in keys), bytes(k[1] for k in keys)
    # the odd entries carry one replaced field: where that is pk.y the compressed key is still the signer's, where it is pk.x the key may not
    # decompress at all - so the expectation is taken on the keys as the device decompresses them, which test_sizes pins on the host mirror
    xy, kok = D.host_decompress_all(x, odd)
    want = bzk.jubjub_verify_batch(xy, msg, sig)
    assert want[0::2] == b"\x01" * (n // 2) and 0 < want.count(1) < n and 0 in kok
    assert all(want[i] == 0 for i in range(n) if not kok[i])
    assert bzk.jubjub_verify_batch_compressed(x, odd, msg, sig) == want
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    d = [_dev(b) for b in (x, odd, msg, sig)]
    torch.cuda.synchronize()
    bzk.jubjub_verify_batch_compressed_dev(d[0], d[1], d[2], d[3], n, ok)
    bzk.sync()
    assert bytes(ok.cpu().numpy().tobytes()) == want


def test_transaction_list(bzk):
    cases = D.tx_list()
    blob = b"".join(D.enc_tx(c[1]) for c in cases)
    want = (bytes(c[2] for c in cases), b"".join(c[3] for c in cases))
    assert L.host_mpn_tx_verify_batch(blob, len(cases)) == want
    got = bzk.mpn_tx_verify_batch(blob, len(cases))
    assert got == want, [(i, c[0]) for i, c in enumerate(cases) if got[0][i] != c[2]]
    assert bzk.mpn_tx_verify_batch(blob, len(cases), want_hash=False) == (want[0], None)
    with pytest.raises(L.BzkError, match="record"):
        bzk.mpn_tx_verify_batch(blob[:-1], len(cases))


def test_transaction_bulk_across_a_staging_chunk(bzk):
    """2^16 transactions are staged per round: 70 000 records need two, the second one short; three record lengths mixed"""
    n = 70000
    txs = D.tx_bulk(n, 31)
    recs = [D.enc_tx(t) for t in txs]
    assert {len(r) for r in recs} >= {190, 254}
    blob = b"".join(recs)
    want = L.host_mpn_tx_verify_batch(blob, n)
    assert 0.6 * n < want[0].count(1) < 0.75 * n and want[1].count(bytes(32)) > 0
    got = bzk.mpn_tx_verify_batch(blob, n)
    assert got[0] == want[0], [i for i in range(n) if got[0][i] != want[0][i]][:10]
    assert got[1] == want[1]


def test_scalars_that_are_not_residues(bzk):
    t = D.tx_list()[0][1]
    blob = D.enc_tx(t)
    txs = [blob[:off] + bad + blob[off + 32:] for off in (4, 37, 74, 126, 158, 190) for bad in (D.R_LIMBS, D.ALL_ONES)]
    allb = blob + b"".join(txs)
    assert bzk.mpn_tx_verify_batch(allb, 1 + len(txs)) == L.host_mpn_tx_verify_batch(allb, 1 + len(txs))


def test_device_admission_makes_the_same_work_and_its_proof_verifies(bzk):
    good = D.wire_transfers()
    bad = D.bad_transfers(good)
    mixed = good[:2] + [bad[0]] + good[2:5] + [bad[1]] + good[5:] + [bad[2]]
    want, want_root = D.twin_work()
    host, dev = D.admission_world(), D.admission_world(bzk)
    bzk.prof_enable(True)
    bzk.prof_reset()
    try:
        got_dev = D.admit(dev, mixed)
        bzk.sync()
        launches, _ = bzk.prof_query("jubjub_decompress")
    finally:
        bzk.prof_enable(False)
    assert launches == 1  # one decompress launch covers the 2 n keys
    assert got_dev == D.admit(host, mixed) == (bytes(0 if any(t is b for b in bad) else 1 for t in mixed), len(good))
    wd = dev.make_work(2, sc.VKS, 10, log4_batches=(1, 1, 2)).encode()
    assert wd == host.make_work(2, sc.VKS, 10, log4_batches=(1, 1, 2)).encode() == want.encode()
    assert dev.root() == host.root() == want_root
    # one proof over a work admitted on the device, in the small shape the worker tests prove
    keys = W.DevSetup(bzk, {k: fr_bytes(fr_list(5, 9000 + k)) for k in range(3)})
    try:
        vks = [keys.keys(k, 3, 3, 1)[1] for k in range(3)]
        small = D.admission_world(bzk)
        assert D.admit(small, [good[0], bad[0], good[1], good[2]]) == (b"\x01\x00\x01\x01", 3)
        blob = small.make_work(2, vks, 300).encode()
        worker = W.Worker(bzk, ALICE, ("127.0.0.1", 9), keys)
        work = L.MpnWork.decode(blob)
        proof = worker.prove(work)
        assert proof is not None and len(proof) == 387 and work.verify(ALICE, proof)
    finally:
        keys.close()
