"""Wire-form L1 transactions with ctx = NULL (bzk_l1_tx_verify_batch, bzk_sha3_merkle_roots, bzk_block_bodies_check): the host path runs the
per-lane code of the device kernels (bzk_gather.cuh, bzk_l1.cuh), so what is checked here is the parser, the gathered message's piece list under
both hashes, and the tree's layout.  Expected values: tests/l1_tx_cases.py (decode, set Unsigned / None, re-encode, hashlib and the Ed25519
restatement; a restatement of merkle.rs pinned on the reference's vectors).  The device run: tests/test_gpu_l1_admit.py."""
import ctypes as C
import hashlib
import struct

import pytest

import bincode_ref as B
import l1_tx_cases as X
from bazuka_amd import lib as L

BZK_OK, BZK_E_ARG = 0, -1


def _check(records, form=X.FORM_TX, prefixed=False):
    want_ok, want_hash = X.expected_batch(records, form, prefixed)
    ok, h = L.host_l1_tx_verify_batch(b"".join(records), len(records), form)
    assert ok == want_ok, [i for i in range(len(records)) if ok[i] != want_ok[i]]
    assert h == want_hash, [i for i in range(len(records)) if h[32 * i:32 * i + 32] != want_hash[32 * i:32 * i + 32]]
    return ok, h


def test_merkle_restatement_reproduces_the_reference_vectors():
    for v in X.reference_merkle_vectors():
        leaves = [hashlib.sha3_256(bytes([i])).digest() for i in range(v["first"], v["first"] + v["count"])]
        assert X.merkle_root(leaves) == bytes(v["root"]), v


def test_signed_form_is_what_the_restatement_says():
    """the test data's own layout: the product's splice and the restatement's re-encoding describe the same bytes"""
    for tx in X.variant_txs():
        lay, rec = X.layout(tx), X.enc(tx)
        a, b = lay["cut"] if lay["cut"] else (lay["sig_tag"], lay["sig_tag"])
        spliced = rec[:a] + (b"\x00" + rec[b:lay["sig_tag"]] if lay["cut"] else b"") + bytes(4)
        assert spliced == X.signed_bytes(tx), tx["data"][0]
        assert rec[lay["key"]:lay["key"] + 32] == tx["src"] and rec[lay["sig"]:] == tx["sig"][1]


@pytest.mark.parametrize("form", [X.FORM_TX, X.FORM_TX_AND_DELTA])
def test_corpus(form):
    corpus = X.corpus(form)
    ok, h = _check([r for _, r in corpus], form)
    verdict = {label: ok[i] for i, (label, _) in enumerate(corpus)}
    hashes = {label: h[32 * i:32 * i + 32] for i, (label, _) in enumerate(corpus)}
    for tx in X.variant_txs():
        name = tx["data"][0]
        assert verdict[f"variant {name}"] == 1 and verdict[f"{name}: src None"] == 1
        for bad in ("Unsigned", "wrong signature", "wrong key", "flip in the first signed region", "flip in the last signed region"):
            assert verdict[f"{name}: {bad}"] == 0, (name, bad)
        assert hashes[f"{name}: Unsigned"] == hashes[f"variant {name}"] == hashes[f"{name}: wrong signature"]  # the signature is not hashed
        assert hashes[f"{name}: flip in the first signed region"] != hashes[f"variant {name}"]
        if name in ("CreateContract", "UpdateContract"):  # bytes outside the signature: neither verdict nor hash moves
            label = f"{name}: flip inside the Some(..) the signature leaves out"
            assert verdict[label] == 1 and hashes[label] == hashes[f"variant {name}"]
            assert verdict[f"{name}: flip in the fee, after the cut"] == 0
        if form == X.FORM_TX_AND_DELTA:
            label = f"{name}: flip in the trailing state_delta"
            assert verdict[label] == 1 and hashes[label] == hashes[f"variant {name}"]


def test_each_record_alone_gives_the_batch_verdict():
    for label, rec in X.corpus()[:14]:
        want = X.expected(rec)
        assert L.host_l1_tx_verify_batch(rec, 1) == (bytes([want[0]]), want[1]), label
        assert L.host_l1_tx_verify_batch(rec, 1, want_hash=False) == (bytes([want[0]]), None), label


def test_cut_alignment():
    recs = X.cut_sweep()
    residues = set()
    for rec in recs[:16]:
        tx = B.decode(X.schema(X.FORM_TX), rec)
        residues.add(X.layout(tx)["cut"][0] % 8)
    assert residues == set(range(8))  # the None byte lands on every position of a word
    ok, _ = _check(list(recs))
    assert ok == b"\x01" * len(recs)


def test_padding_edges():
    recs = X.memo_sweep()
    lens = [X.layout(B.decode(X.schema(X.FORM_TX), r))["sig_tag"] + 4 for r in recs]
    assert {(64 + k) % 128 for k in lens} == set(range(128)) and {k % 136 for k in lens} == set(range(136))
    ok, _ = _check(list(recs))
    assert ok == b"\x01" * len(recs)


def test_length_prefixed_signatures_under_the_wire_flag():
    recs = [r for _, r in X.corpus(X.FORM_TX, True)[:21]]
    plain = [r for _, r in X.corpus()[:21]]
    assert len(recs[0]) == len(plain[0]) + 8 and len(recs[6]) == len(plain[6]) + 16  # UpdateContract carries a ContractDeposit's signature too
    want_ok, want_hash = X.expected_batch(recs, X.FORM_TX, True)
    L.mpn_set_wire_flags(1)
    try:
        got = L.host_l1_tx_verify_batch(b"".join(recs), len(recs))
        with pytest.raises(L.BzkError):
            L.host_l1_tx_verify_batch(b"".join(plain), len(plain))
    finally:
        L.mpn_set_wire_flags(0)
    assert got == (want_ok, want_hash)
    assert want_ok[:7] == b"\x01" * 7
    with pytest.raises(L.BzkError):
        L.host_l1_tx_verify_batch(b"".join(recs), len(recs))


# ---- refusals
def _refused(blob, n, form=X.FORM_TX):
    """BZK_E_ARG, nothing written; returns the error text"""
    lib = L.load_library()
    ok, h = C.create_string_buffer(b"\x07" * n, n), C.create_string_buffer(b"\x07" * 32 * n, 32 * n)
    st = lib.bzk_l1_tx_verify_batch(None, blob, len(blob), n, form, ok, h)
    assert st == BZK_E_ARG, st
    assert ok.raw == b"\x07" * n and h.raw == b"\x07" * 32 * n
    return lib.bzk_mpn_work_last_error().decode()


def _update_contract():
    return X.variant_txs()[6]


def test_truncation_is_refused_at_every_length():
    """every proper prefix of a good record followed by an UpdateContract record: every field boundary of it is among them"""
    first, rec = X.enc(X.variant_txs()[4]), X.enc(_update_contract())
    assert L.host_l1_tx_verify_batch(first + rec, 2)[0] == b"\x01\x01"
    for k in range(len(rec)):
        why = _refused(first + rec[:k], 2)
        assert "record 1" in why, (k, why)
    for k in (0, 1, 40, len(first) - 1):
        assert "record 0" in _refused(first[:k], 1)


def test_trailing_bytes_are_refused():
    rec = X.enc(_update_contract())
    assert "record 0" in _refused(rec + b"\x00", 1) and "after the last record" in _refused(rec + b"\x00", 1)
    assert "record 1" in _refused(rec + rec + b"\x01\x02", 2)
    assert _refused(rec, 0)  # bytes but no records
    assert "record 0" in _refused(X.enc(_update_contract(), X.FORM_TX_AND_DELTA), 1)  # the wrong form leaves its Option behind
    assert "record 0" in _refused(rec, 1, X.FORM_TX_AND_DELTA)


def _with_u32(rec, at, v):
    return rec[:at] + struct.pack("<I", v) + rec[at + 4:]


def test_enum_tags_out_of_range_are_refused():
    uc, cc = _update_contract(), X.variant_txs()[5]
    for tx in (uc, cc, X.variant_txs()[0]):
        lay, rec = X.layout(tx), X.enc(tx)
        assert "TransactionData variant" in _refused(_with_u32(rec, lay["data_tag"], 7), 1)
        assert "Signature variant" in _refused(_with_u32(rec, lay["sig_tag"], 2), 1)
        assert "ContractId variant" in _refused(_with_u32(rec, lay["fee"], 3), 1)
    lay, rec = X.layout(uc), X.enc(uc)
    cid = lay["data_tag"] + 4
    assert rec[cid:cid + 4] == struct.pack("<I", 2)
    assert "ContractId variant" in _refused(_with_u32(rec, cid, 3), 1)
    upd0 = cid + 36 + 8  # contract_id Custom, updates' length
    assert "ContractUpdateData variant" in _refused(_with_u32(rec, upd0 + 4, 4), 1)
    # the first update's ZkProof tag: 391 bytes before its end
    first_update = uc["data"][1]["updates"][0]
    one = X.enc(dict(uc, data=("UpdateContract", dict(uc["data"][1], updates=[first_update], delta=None))))
    none = X.enc(dict(uc, data=("UpdateContract", dict(uc["data"][1], updates=[], delta=None))))
    proof_tag = upd0 + (len(one) - len(none)) - 391
    assert rec[proof_tag:proof_tag + 4] == bytes(4)
    assert "ZkProof variant" in _refused(_with_u32(rec, proof_tag, 1), 1)
    lay, rec = X.layout(cc), X.enc(cc)
    model = lay["data_tag"] + 4 + 40
    assert rec[model:model + 4] == struct.pack("<I", 1)
    assert "ZkStateModel variant" in _refused(_with_u32(rec, model, 3), 1)
    vk = model + len(B.encode(X.ZkStateModel, cc["data"][1]["contract"]["state_model"])) + 8
    assert "ZkVerifierKey variant" in _refused(_with_u32(rec, vk, 1), 1)


def test_option_tags_and_lengths_are_refused():
    uc = _update_contract()
    lay, rec = X.layout(uc), X.enc(uc)
    assert "Option<src> tag" in _refused(b"\x02" + rec[1:], 1)
    assert "Option<ZkDeltaPairs> tag" in _refused(rec[:lay["cut"][0]] + b"\x02" + rec[lay["cut"][0] + 1:], 1)
    both = X.enc(uc, X.FORM_TX_AND_DELTA, state_delta=None)
    assert "Option<state_delta> tag" in _refused(both[:-1] + b"\x02", 1, X.FORM_TX_AND_DELTA)
    short_key = b"\x01" + struct.pack("<Q", 31) + rec[9:9 + 31] + rec[41:]  # a 31-byte key
    assert "public key length" in _refused(short_key, 1)
    assert "public key length" in _refused(rec[:1] + struct.pack("<Q", 33) + rec[9:], 1)
    huge = rec[:lay["sig_tag"] - 8 - len(uc["memo"])] + struct.pack("<Q", 1 << 62) + rec[lay["sig_tag"] - len(uc["memo"]):]
    assert "record 0" in _refused(huge, 1)  # a length that overflows the record
    L.mpn_set_wire_flags(1)
    try:
        pre = X.enc(X.variant_txs(True)[1], X.FORM_TX, True)
        assert "signature length" in _refused(pre[:-72] + struct.pack("<Q", 63) + pre[-64:], 1)
    finally:
        L.mpn_set_wire_flags(0)


def test_record_length_limit():
    """a record of 2^20 bytes is taken, one byte more is refused: no block can carry it (max_block_size)"""
    base = X.tx_of(("RegularSend", {"entries": []}), memo="")
    pad = X.RECORD_MAX - len(X.enc(base))
    at_limit, over = X.enc(dict(base, memo="z" * pad)), X.enc(dict(base, memo="z" * (pad + 1)))
    assert len(at_limit) == X.RECORD_MAX and len(over) == X.RECORD_MAX + 1
    want = X.expected(at_limit)
    assert L.host_l1_tx_verify_batch(at_limit, 1) == (b"\x01", want[1])  # src None
    why = _refused(X.enc(X.variant_txs()[4]) + over, 2)
    assert "record 1" in why and "1048576" in why


def test_argument_checks():
    lib = L.load_library()
    rec = X.enc(X.variant_txs()[4])
    ok, h = C.create_string_buffer(1), C.create_string_buffer(32)
    assert lib.bzk_l1_tx_verify_batch(None, rec, len(rec), 1, 2, ok, h) == BZK_E_ARG  # a bad form
    assert lib.bzk_l1_tx_verify_batch(None, rec, len(rec), 1, 0, None, h) == BZK_E_ARG
    assert lib.bzk_l1_tx_verify_batch(None, None, 0, 0, 0, None, None) == BZK_OK  # n = 0 is a no-op
    assert lib.bzk_sha3_merkle_roots(None, None, None, 0, None, None) == BZK_OK
    assert lib.bzk_block_bodies_check(None, None, 0, None, 0, None, None, None, None) == BZK_OK
    cnt = (C.c_uint64 * 1)(1)
    assert lib.bzk_sha3_merkle_roots(None, None, cnt, 1, h, None) == BZK_E_ARG  # a counted leaf without leaves
    assert lib.bzk_block_bodies_check(None, rec, len(rec), cnt, 1, None, h, None, None) == BZK_E_ARG
    assert lib.bzk_sha3_merkle_roots_dev(None, None, None, 1, 0, None, None) == BZK_E_ARG  # the _dev form needs a context


# ---- the block's tree
def _flat(trees):
    return b"".join(b"".join(t) for t in trees), [len(t) for t in trees]


@pytest.mark.parametrize("i", range(len(X.MERKLE_COUNTS)), ids=[str(c) for c in X.MERKLE_COUNTS])
def test_merkle_tree_alone(i):
    leaves = X.merkle_trees()[i]
    want = X.merkle_nodes(list(leaves))
    roots, nodes = L.host_sha3_merkle_roots(b"".join(leaves), [len(leaves)], want_nodes=True)
    assert roots == want[0] and nodes == b"".join(want)
    assert L.host_sha3_merkle_roots(b"".join(leaves), [len(leaves)]) == want[0]


def test_merkle_twelve_trees_in_one_call():
    trees = X.merkle_trees()
    flat, counts = _flat(trees)
    want = [X.merkle_nodes(list(t)) for t in trees]
    roots, nodes = L.host_sha3_merkle_roots(flat, counts, want_nodes=True)
    assert roots == b"".join(w[0] for w in want)
    assert nodes == b"".join(b"".join(w) for w in want)
    assert roots[:32] == bytes(32) and roots[32:64] == trees[1][0]  # no leaves: zeros; one leaf: the leaf


def test_merkle_equal_children():
    leaf = hashlib.sha3_256(b"same").digest()
    for n in (2, 5, 8):
        want = X.merkle_nodes([leaf] * n)
        assert L.host_sha3_merkle_roots(leaf * n, [n], want_nodes=True) == (want[0], b"".join(want)), n


def test_merkle_reference_vectors():
    vs = X.reference_merkle_vectors()
    trees = [[hashlib.sha3_256(bytes([i])).digest() for i in range(v["first"], v["first"] + v["count"])] for v in vs]
    flat, counts = _flat(trees)
    assert L.host_sha3_merkle_roots(flat, counts) == b"".join(bytes(v["root"]) for v in vs)


# ---- block bodies
def test_block_bodies_check():
    txs, counts, records = X.bodies()
    want = X.bodies_expected()
    assert want[0] == bytes(0 if j == X.BAD_BODY else 1 for j in range(len(counts)))  # only the body with the bad signature fails; the empty one passes
    assert want[1][:32] == bytes(32) and want[1][32:64] == want[3][:32]
    got = L.host_block_bodies_check(txs, list(counts))
    assert got == want
    sig_ok, roots, tx_ok, hashes = L.host_block_bodies_check(txs, list(counts), want_tx=False)
    assert (sig_ok, roots) == want[:2] and tx_ok is None and hashes is None
    with pytest.raises(L.BzkError, match="record"):
        L.host_block_bodies_check(txs[:-1], list(counts))
    with pytest.raises(L.BzkError):
        L.host_block_bodies_check(txs, [0, 1, 3, 64])  # the counts leave a record over
