"""Wire-form deposit admission (bzk_mpn_deposit_verify_batch, bzk_mpn_push_deposits) with ctx = NULL: the parser's refusals, the two verdict bits
against the restatement tests/ed25519_cases.py and the key decompression of tests/decompress_cases.py, payments whose signed bytes end on SHA-512's
padding and block edges, and admission against a world fed the same deposits through bzk_mpn_push_deposit.  The host path runs the per-lane code
of the device kernels (tests/test_ed25519_cpu.py runs it with its assertions on).  The device run: tests/test_gpu_deposit_admit.py."""
import copy
import ctypes as C
import random
import struct

import pytest

import bincode_ref as B
import decompress_cases as Dc
import ed25519_cases as E
import r1cs_scenarios as sc
import withdraw_cases as Wd
from bazuka_amd import lib as L

BZK_OK, BZK_E_ARG = 0, -1
PROVER = bytes(range(1, 33))
BATCHES = (2, 1, 1)


def _addr_bytes(rec) -> bytes:
    xy = Dc.oracle_decompress(rec["mpn_address"]["x"], rec["mpn_address"]["odd"])
    return bytes(64) if xy is None else Wd.F(xy[0]) + Wd.F(xy[1])


def _oracle_bits(rec) -> int:
    return (1 if E.oracle_signature(rec) else 0) | (2 if _addr_bytes(rec) != bytes(64) else 0)


@pytest.fixture(scope="module")
def records():
    return E.admission_records()


def test_record_layout(records):
    r = E.signed_deposit(b"w", E.account_address(0), "", E.ZIESHA, E.ZIESHA, 1)
    assert len(E.enc(r)) == 33 + 117 + 64 and len(E.unsigned_bytes(r)) == 117  # the shortest record without a signature: 150 bytes
    assert E.unsigned_bytes(r) == E.payment_bytes(r)[:116] + b"\x00" and E.payment_bytes(r)[116] == 1
    assert len(E.enc(r, prefixed=True)) == len(E.enc(r)) + 8
    assert L.host_mpn_deposit_verify_batch(E.enc(r), 1) == (b"\x03", _addr_bytes(r))


def test_malformed_records_are_refused(records):
    lib = L.load_library()
    recs = [E.enc(r) for r in records[:3]]
    blob, n = b"".join(recs), 3
    ok, xy = C.create_string_buffer(b"\x07" * n, n), C.create_string_buffer(b"\x07" * 64 * n, 64 * n)

    def run(b, k=n):
        st = lib.bzk_mpn_deposit_verify_batch(None, b, len(b), k, ok, xy)
        assert st == BZK_OK or (ok.raw == b"\x07" * n and xy.raw == b"\x07" * 64 * n)  # nothing is written on a refusal
        return st, lib.bzk_mpn_work_last_error().decode()

    st, why = run(blob[:-1])
    assert st == BZK_E_ARG and "record 2" in why, why                                    # a truncated last record
    st, why = run(blob + b"\x00")
    assert st == BZK_E_ARG and "after the last record" in why, why
    tag_at = len(recs[0]) + len(recs[1]) - 65                                            # record 1: the Option<Signature> tag
    assert blob[tag_at] == 1
    st, why = run(blob[:tag_at] + b"\x02" + blob[tag_at + 1:])
    assert st == BZK_E_ARG and "Option tag" in why and "record 1" in why, why
    l1_at = 33 + 8 + len("deposit 0") + 36 + 4 + 32                                      # record 0: the L1 key's length
    assert blob[l1_at:l1_at + 8] == struct.pack("<Q", 32)
    st, why = run(blob[:l1_at] + struct.pack("<Q", 31) + blob[l1_at + 8:])
    assert st == BZK_E_ARG and "ed25519 public key length" in why and "record 0" in why, why
    assert run(blob, 4)[0] == BZK_E_ARG and run(blob, 2)[0] == BZK_E_ARG                  # a count the bytes do not hold
    # the longest payment taken is 65 536 bytes
    fits = E.signed_deposit(b"long", E.account_address(1), "L" * (65536 - 181), E.ZIESHA, E.ZIESHA, 5)
    over = E.signed_deposit(b"long", E.account_address(1), "L" * (65537 - 181), E.ZIESHA, E.ZIESHA, 5)
    assert len(E.payment_bytes(fits)) == 65536 and len(E.payment_bytes(over)) == 65537
    assert L.host_mpn_deposit_verify_batch(recs[0] + E.enc(fits), 2)[0] == b"\x03\x03"
    st, why = run(recs[0] + E.enc(over), 2)
    assert st == BZK_E_ARG and "65536" in why and "record 1" in why, why
    assert run(blob)[0] == BZK_OK and ok.raw == b"\x03\x03\x03"
    assert lib.bzk_mpn_deposit_verify_batch(None, None, 0, 0, None, None) == BZK_OK
    assert lib.bzk_mpn_deposit_verify_batch(None, None, 0, 1, ok, None) == BZK_E_ARG
    assert lib.bzk_mpn_deposit_verify_batch(None, blob, len(blob), n, None, None) == BZK_E_ARG
    w = Wd.admission_world()
    acc = C.c_uint64(99)
    short = blob[:-1]
    assert lib.bzk_mpn_push_deposits(w.h, short, len(short), n, ok, C.byref(acc)) == BZK_E_ARG and acc.value == 0
    assert lib.bzk_mpn_push_deposits(None, blob, len(blob), n, ok, None) == BZK_E_ARG
    with pytest.raises(L.BzkError, match="record 2"):
        w.push_deposits(short, n)
    assert w.push_deposits(b"", 0) == (b"", 0)


def test_verdict_bits_in_all_four_combinations_and_without_a_signature(records):
    rnd = random.Random(31)
    good = records[0]
    bad_sig = copy.deepcopy(good)
    bad_sig["payment"]["amount"]["amount"] += 1
    bad_key = copy.deepcopy(good)
    bad_key["mpn_address"]["x"] = Dc.no_root_x(rnd)
    both = copy.deepcopy(bad_sig)
    both["mpn_address"]["x"] = Dc.R_LIMBS
    unsigned = copy.deepcopy(good)
    unsigned["payment"]["sig"] = None
    other_signer = copy.deepcopy(good)
    other_signer["payment"]["src"] = E.public_key(b"someone else")
    batch = [good, bad_sig, bad_key, both, unsigned, other_signer, records[1]]
    want = bytes(_oracle_bits(r) for r in batch)
    assert want == bytes([3, 2, 1, 0, 2, 2, 3])
    ok, xy = L.host_mpn_deposit_verify_batch(b"".join(E.enc(r) for r in batch), len(batch))
    assert ok == want and xy == b"".join(_addr_bytes(r) for r in batch)
    assert L.host_mpn_deposit_verify_batch(b"".join(E.enc(r) for r in batch), len(batch), want_address=False) == (want, None)


@pytest.mark.parametrize("memo_len", [58, 59, 74, 75, 76])
def test_memo_lengths_at_the_padding_edges(memo_len):
    """R | A | unsigned payment is 181 + memo bytes with Ziesha ids: 239, 240 (the length words no longer fit the block), 255, 256, 257"""
    r = E.signed_deposit(b"edge %d" % memo_len, E.account_address(2), "e" * memo_len, E.ZIESHA, E.ZIESHA, 9, E.ZIESHA, 1)
    assert 64 + len(E.unsigned_bytes(r)) == 181 + memo_len and (181 + memo_len) % 128 in (111, 112, 127, 0, 1)
    flipped = copy.deepcopy(r)
    flipped["payment"]["memo"] = "e" * (memo_len - 1) + "f"
    assert L.host_mpn_deposit_verify_batch(E.enc(r) + E.enc(flipped), 2)[0] == bytes([_oracle_bits(r), _oracle_bits(flipped)]) == b"\x03\x02"


def test_length_prefixed_signatures_follow_the_wire_flag(records):
    blob = b"".join(E.enc(r, prefixed=True) for r in records[:2])
    with pytest.raises(L.BzkError):
        L.host_mpn_deposit_verify_batch(blob, 2)
    L.mpn_set_wire_flags(1)
    try:
        assert L.host_mpn_deposit_verify_batch(blob, 2)[0] == b"\x03\x03"
    finally:
        L.mpn_set_wire_flags(0)
    with pytest.raises(L.BzkError):
        L.mpn_set_wire_flags(2)


def _world_a(which):
    a = Wd.admission_world()
    for acct, amount in which:
        a.push_deposit(acct, Wd.ZIESHA_ID, amount)
    return a, a.make_work(0, sc.VKS, 10, log4_batches=BATCHES)


def test_host_admission_equals_push_deposit_and_refuses_exactly_what_the_restatement_refuses(records):
    rnd = random.Random(32)
    a, awork = _world_a(E.DEPOSITS)
    bad_sig = copy.deepcopy(records[1])
    bad_sig["payment"]["nonce"] += 1
    unsigned = copy.deepcopy(records[2])
    unsigned["payment"]["sig"] = None
    no_addr = copy.deepcopy(records[3])
    no_addr["mpn_address"]["x"] = Dc.no_root_x(rnd)
    wrong_id = E.signed_deposit(b"w1", E.account_address(1), "", E.custom(E.MPN_CONTRACT + 1), E.ZIESHA, 5)   # signed and well-addressed
    circuit1 = E.signed_deposit(b"w2", E.account_address(1), "", E.custom(E.MPN_CONTRACT), E.ZIESHA, 5, circuit=1)
    bad_token = E.signed_deposit(b"w3", E.account_address(1), "", E.custom(E.MPN_CONTRACT), ("Custom", Dc.R_LIMBS), 5)
    bad = [bad_sig, unsigned, no_addr, wrong_id, circuit1, bad_token]
    assert L.host_mpn_deposit_verify_batch(b"".join(E.enc(r) for r in bad), len(bad))[0] == bytes([2, 2, 1, 3, 3, 3])
    mixed = records[:1] + bad[:2] + records[1:3] + bad[2:5] + records[3:] + bad[5:]
    want = bytes(1 if E.oracle_admits(r) else 0 for r in mixed)
    assert want == bytes(0 if any(r is b for b in bad) else 1 for r in mixed)
    b = Wd.admission_world()
    b.set_threads(3)
    ok, accepted = b.push_deposits(b"".join(E.enc(r) for r in mixed), len(mixed))
    assert ok == want and accepted == len(records)
    bwork = b.make_work(0, sc.VKS, 10, log4_batches=BATCHES)
    # the same root and the same public inputs as the world fed through bzk_mpn_push_deposit
    assert b.root() == a.root()
    assert (bwork.height, bwork.state, bwork.aux_data, bwork.next_state, bwork.new_root_hash) == \
           (awork.height, awork.state, awork.aux_data, awork.next_state, awork.new_root_hash)
    # the work decodes and carries each payment as received, in input order
    blob = bwork.encode()
    decoded = L.MpnWork.decode(blob)
    assert decoded.encode() == blob and decoded.n_transitions == awork.n_transitions
    kind, transitions = B.decode(B.MpnWork, blob)["data"]
    assert kind == "Deposit" and [t["tx"] for t in transitions if t["enabled"]] == records
    r = decoded.synthesize(PROVER)
    assert r.satisfied and (r.accepted, r.rejected) == (len(records), 0)
    ra = L.MpnWork.decode(awork.encode()).synthesize(PROVER)
    assert ra.satisfied and (ra.accepted, ra.rejected) == (r.accepted, r.rejected)
