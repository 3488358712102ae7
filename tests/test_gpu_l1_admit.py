"""Wire-form L1 transactions on the GPU (bzk_l1_tx_verify_batch, bzk_sha3_merkle_roots / _dev, bzk_block_bodies_check): the device against the
ctx = NULL path and against the restatements of tests/l1_tx_cases.py, which tests/test_l1_admit_cpu.py pins.  Batch sizes 1, 64, 65 and 257 are
one lane, a full wavefront, one lane into the next, and past one 256-lane block of the hash kernel.  No build of the library lowers the chunk
size, so no batch here crosses a chunk end (2^16 records); tools/l1_admit_bench.py's largest rows do and compare with the host path."""
import ctypes as C

import pytest
import torch

import l1_tx_cases as X
from bazuka_amd import lib as L

pytestmark = pytest.mark.gpu
SIZES = [1, 64, 65, 257]


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


_want = {}


def _expected(form):
    """the corpus' records with the restatement's verdicts and hashes, computed once"""
    if form not in _want:
        recs = [r for _, r in X.corpus(form)]
        _want[form] = (recs,) + X.expected_batch(recs, form)
    return _want[form]


@pytest.mark.parametrize("form", [X.FORM_TX, X.FORM_TX_AND_DELTA])
@pytest.mark.parametrize("n", SIZES)
def test_corpus_device_host_and_restatement_agree(bzk, form, n):
    recs, ok, h = _expected(form)
    pick = [(7 * i + n) % len(recs) for i in range(n)]  # the corpus cycled, so every lane of a wave holds another kind of record
    blob = b"".join(recs[k] for k in pick)
    want = (bytes(ok[k] for k in pick), b"".join(h[32 * k:32 * k + 32] for k in pick))
    assert bzk.l1_tx_verify_batch(blob, n, form) == want
    assert L.host_l1_tx_verify_batch(blob, n, form) == want
    assert bzk.l1_tx_verify_batch(blob, n, form, want_hash=False) == (want[0], None)


def test_memo_sweep_in_one_batch(bzk):
    recs = list(X.memo_sweep())
    want = X.expected_batch(recs)
    assert want[0] == b"\x01" * len(recs)
    assert bzk.l1_tx_verify_batch(b"".join(recs), len(recs)) == want


def test_cut_alignment_sweep_in_one_batch(bzk):
    recs = list(X.cut_sweep())
    want = X.expected_batch(recs)
    assert want[0] == b"\x01" * len(recs)
    assert bzk.l1_tx_verify_batch(b"".join(recs), len(recs)) == want


def test_length_prefixed_signatures_under_the_wire_flag(bzk):
    recs = [r for _, r in X.corpus(X.FORM_TX, True)[:21]]
    want = X.expected_batch(recs, X.FORM_TX, True)
    L.mpn_set_wire_flags(1)
    try:
        assert bzk.l1_tx_verify_batch(b"".join(recs), len(recs)) == want
    finally:
        L.mpn_set_wire_flags(0)


def test_merkle_twelve_trees_host_and_dev_forms(bzk):
    trees = X.merkle_trees()
    flat, counts = b"".join(b"".join(t) for t in trees), [len(t) for t in trees]
    want = [X.merkle_nodes(list(t)) for t in trees]
    want_roots, want_nodes = b"".join(w[0] for w in want), b"".join(b"".join(w) for w in want)
    assert bzk.sha3_merkle_roots(flat, counts, want_nodes=True) == (want_roots, want_nodes)
    assert bzk.sha3_merkle_roots(flat, counts) == want_roots
    for i in (0, 1, 2, 9, 11):  # a tree alone: no leaves, the leaf itself, one level, a ragged and the deepest one
        assert bzk.sha3_merkle_roots(b"".join(trees[i]), [counts[i]]) == want[i][0], counts[i]
    leaves, cnt = _dev(flat), torch.tensor(counts, dtype=torch.int64).cuda()
    roots = torch.full((32 * len(counts),), 7, dtype=torch.uint8, device="cuda")
    nodes = torch.full((len(want_nodes),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bzk.sha3_merkle_roots_dev(leaves, cnt, len(counts), sum(counts), roots, nodes)
    bzk.sync()
    assert bytes(roots.cpu().numpy().tobytes()) == want_roots and bytes(nodes.cpu().numpy().tobytes()) == want_nodes
    roots.fill_(7)
    torch.cuda.synchronize()
    bzk.sha3_merkle_roots_dev(leaves, cnt, len(counts), sum(counts), roots)  # without nodes_out: the trees live in the workspace
    bzk.sync()
    assert bytes(roots.cpu().numpy().tobytes()) == want_roots


def test_merkle_equal_children(bzk):
    leaf = bytes(range(32))
    for n in (2, 5, 8):
        want = X.merkle_nodes([leaf] * n)
        assert bzk.sha3_merkle_roots(leaf * n, [n], want_nodes=True) == (want[0], b"".join(want)), n


def test_block_bodies_check(bzk):
    txs, counts, _ = X.bodies()
    want = X.bodies_expected()
    assert bzk.block_bodies_check(txs, list(counts)) == want
    assert bzk.block_bodies_check(txs, list(counts), want_tx=False) == want[:2] + (None, None)
    assert L.host_block_bodies_check(txs, list(counts)) == want
    assert bzk.block_bodies_check(b"", [0, 0]) == (b"\x01\x01", bytes(64), b"", b"")  # empty bodies only


def test_argument_checks(bzk):
    lib, h = bzk.lib, bzk.h
    rec = X.enc(X.variant_txs()[4])
    ok, out = C.create_string_buffer(b"\x07", 1), C.create_string_buffer(b"\x07" * 32, 32)
    assert lib.bzk_l1_tx_verify_batch(h, rec, len(rec), 1, 2, ok, out) == -1  # a bad form
    assert lib.bzk_l1_tx_verify_batch(h, rec, len(rec), 1, 0, None, out) == -1
    assert lib.bzk_l1_tx_verify_batch(h, rec[:-1], len(rec) - 1, 1, 0, ok, out) == -1 and b"record 0" in lib.bzk_mpn_work_last_error()
    assert ok.raw == b"\x07" and out.raw == b"\x07" * 32  # nothing is written on a refusal
    assert lib.bzk_l1_tx_verify_batch(h, None, 0, 0, 0, None, None) == 0  # n = 0 is a no-op
    assert lib.bzk_sha3_merkle_roots(h, None, None, 0, None, None) == 0
    assert lib.bzk_sha3_merkle_roots_dev(h, None, None, 0, 0, None, None) == 0
    assert lib.bzk_block_bodies_check(h, None, 0, None, 0, None, None, None, None) == 0
    cnt = (C.c_uint64 * 1)(1)
    assert lib.bzk_block_bodies_check(h, rec, len(rec), cnt, 1, None, out, None, None) == -1
    assert lib.bzk_sha3_merkle_roots_dev(h, None, None, 1, 0, None, None) == -1
    assert lib.bzk_l1_tx_verify_batch(h, rec, len(rec), 1, 0, ok, None) == 0 and ok.raw == b"\x01"  # hash_out may be NULL
