"""Device SHA3-256, hash_to_scalar and wire-form withdrawal admission (bazuka_amd/csrc/bzk_keccak.cuh, bzk_mpn_withdraw_verify_batch,
bzk_mpn_push_withdraws) on the CPU.  The kernel's per-lane functions - sha3_256_one with its blanked range and fr_from_le_bytes_mod - run through
tests/host/keccak_check.hip (bound assertions on: one that fires aborts the process) and are compared with hashlib and Python integers.  Then the host
path of the two withdrawal entries: the parser, the verdict bits and fingerprints against the independent route of tests/withdraw_cases.py, and
admission against a world fed through bzk_mpn_push_withdraw.  The device run: tests/test_gpu_withdraw_admit.py."""
import ctypes as C
import hashlib
import os
import random
import struct

import pytest

import bincode_ref as B
import r1cs_scenarios as sc
import withdraw_cases as Wd
from bazuka_amd import lib as L
from oracle import pyref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
R = pr.R_MOD
BZK_OK, BZK_E_ARG = 0, -1
NO_BLANK = 2 ** 64 - 1
PROVER = bytes(range(1, 33))


@pytest.fixture(scope="module")
def harness():
    lib = C.CDLL(os.path.join(ROOT, "tests", "host", "_keccak_check.so"))

    class H:
        @staticmethod
        def sha3(msgs, blank=None, want_scalar=True):
            n = len(msgs)
            off = (C.c_uint64 * (n + 1))()
            for i, m in enumerate(msgs):
                off[i + 1] = off[i] + len(m)
            bl = (C.c_uint64 * n)(*blank) if blank is not None else None
            dig, sc = C.create_string_buffer(32 * n), C.create_string_buffer(32 * n)
            assert lib.kc_sha3_batch(b"".join(msgs) + b"\0", off, bl, C.c_uint64(n), dig, sc if want_scalar else None) == 0
            return dig.raw, sc.raw

        @staticmethod
        def scalar_new(vals: bytes):
            out = C.create_string_buffer(len(vals))
            assert lib.kc_scalar_new_batch(vals, C.c_uint64(len(vals) // 32), out) == 0
            return out.raw
    return H


# ---- SHA3-256 and ZkScalar::new
def test_digest_literals(harness):
    dig, _ = harness.sha3([b"", b"abc"])
    assert dig[:32].hex() == "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a"
    assert dig[32:].hex() == "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532"


def test_every_length_to_300_and_one_long_message(harness):
    msgs = Wd.messages(list(range(301)) + [65536], 11)
    dig, sc = harness.sha3(msgs)
    for i, m in enumerate(msgs):
        want = hashlib.sha3_256(m).digest()
        assert dig[32 * i:32 * i + 32] == want, len(m)
        assert sc[32 * i:32 * i + 32] == Wd.scalar_new(want) == L.host_scalar_new(want), len(m)


@pytest.mark.parametrize("length,at", [(112, 48), (212, 116), (300, 136 - 32), (300, 136), (245, 245 - 32), (272, 240), (32, 0), (5112, 5048)])
def test_blanked_range(harness, length, at):
    """inside one block, across a block edge (116 + 32 > 136), ending at / starting on the edge, ending at the message's end, the whole message"""
    m = Wd.messages([length], 100 + length + at)[0]
    assert any(m[at:at + 32])
    want = hashlib.sha3_256(m[:at] + bytes(32) + m[at + 32:]).digest()
    dig, _ = harness.sha3([m, m], blank=[at, NO_BLANK], want_scalar=False)
    assert dig[:32] == want and dig[32:] == hashlib.sha3_256(m).digest() != want


def test_fr_from_le_bytes_mod(harness):
    rnd = random.Random(12)
    vals = [0, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 2 ** 256 - 1] + [rnd.getrandbits(256) for _ in range(2000)]
    assert sum(v >= 2 * R for v in vals) > 100 and sum(R <= v < 2 * R for v in vals) > 500  # both subtractions are exercised
    raw = b"".join(v.to_bytes(32, "little") for v in vals)
    out = harness.scalar_new(raw)
    for i, v in enumerate(vals):
        got = out[32 * i:32 * i + 32]
        assert U(got) == v % R and got == F(v % R), i
        assert got == L.host_scalar_new(raw[32 * i:32 * i + 32]), i


# ---- records
def test_encoder_gives_the_record_lengths_of_the_wire_format():
    shortest = Wd.signed_withdraw(b"enc", 1, "", Wd.NULL, Wd.ZIESHA, 5, Wd.NULL, 1)
    assert len(Wd.payment_bytes(shortest)) == 112 and len(Wd.enc(shortest)) == 245
    customs = Wd.signed_withdraw(b"enc", 1, "", Wd.custom(77), Wd.custom(4242), 5, Wd.custom(99), 1)
    assert len(Wd.payment_bytes(customs)) == 208 and Wd.calldata_offset(customs) == 48
    cases = Wd.fixed_list()
    assert tuple(len(Wd.payment_bytes(c[1])) for c in cases[:9]) == Wd.PAYMENT_LENGTHS
    off = Wd.calldata_offset(cases[4][1])
    assert off == 116 and off < 136 < off + 32  # the 212-byte payment: calldata across the block edge
    ok, fp = L.host_mpn_withdraw_verify_batch(Wd.enc(shortest) + Wd.enc(customs), 2)
    assert ok == b"\x03\x03" and fp == Wd.oracle_withdraw(shortest)[1] + Wd.oracle_withdraw(customs)[1]


def test_fixed_list_against_the_independent_route():
    cases = Wd.fixed_list()
    assert len(cases) == 9 + 4 * len(Wd.MUTATIONS)
    by = {k: [c[2] for c in cases if c[0] == k] for k in ("valid",) + Wd.MUTATIONS}
    assert by["valid"] == [3] * 9
    assert all(by[k] == [1] * 4 for k in Wd.CALLDATA_ONLY), by
    assert all(by[k] == [2] * 4 for k in Wd.SIGNATURE_SIDE), by
    assert all(by[k] == [0] * 4 for k in Wd.BOTH_FAIL), by
    want = (bytes(c[2] for c in cases), b"".join(c[3] for c in cases))
    blob = b"".join(Wd.enc(c[1]) for c in cases)
    got = L.host_mpn_withdraw_verify_batch(blob, len(cases))
    assert got[0] == want[0], [(i, c[0], got[0][i], c[2]) for i, c in enumerate(cases) if got[0][i] != c[2]]
    assert got[1] == want[1]
    assert L.host_mpn_withdraw_verify_batch(blob, len(cases), want_fingerprint=False) == (want[0], None)
    # a changed calldata leaves the fingerprint alone; a changed memo does not
    k = 9
    for b in (cases[1], cases[2], cases[4], cases[8]):
        for w in Wd.MUTATIONS:
            same = cases[k][3] == b[3]
            assert same == (w not in ("memo byte changed", "amount + 1")), (w, same)
            k += 1


def test_fingerprints_on_the_harness_equal_the_host_entry(harness):
    """the blanked range as the device path uses it: the payment as it stands, calldata's offset, no copy"""
    recs = [c[1] for c in Wd.fixed_list()]
    _, sc = harness.sha3([Wd.payment_bytes(r) for r in recs], blank=[Wd.calldata_offset(r) for r in recs])
    assert sc == b"".join(c[3] for c in Wd.fixed_list())


def test_scalars_that_are_not_residues_are_verdicts_not_errors():
    rec, bad = Wd.non_residue_variants()
    blob = Wd.enc(rec) + b"".join(Wd.enc(r) for r in bad)
    ok, fp = L.host_mpn_withdraw_verify_batch(blob, 1 + len(bad))
    assert ok == b"\x03" + bytes(len(bad))
    assert (ok, fp) == (bytes([Wd.oracle_withdraw(rec)[0]] + [Wd.oracle_withdraw(r)[0] for r in bad]),
                        b"".join(Wd.oracle_withdraw(r)[1] for r in [rec] + bad))


def test_malformed_records_are_refused():
    lib = L.load_library()
    recs = [Wd.enc(c[1]) for c in Wd.fixed_list()[:3]]
    blob, n = b"".join(recs), 3
    ok, fp = C.create_string_buffer(b"\x07" * n, n), C.create_string_buffer(b"\x07" * 32 * n, 32 * n)

    def run(b, k=n):
        st = lib.bzk_mpn_withdraw_verify_batch(None, b, len(b), k, ok, fp)
        assert st == BZK_OK or (ok.raw == b"\x07" * n and fp.raw == b"\x07" * 32 * n)  # nothing is written on a refusal
        return st, lib.bzk_mpn_work_last_error().decode()

    st, why = run(blob[:-1])
    assert st == BZK_E_ARG and "record 2" in why, why                                    # a truncated last record
    st, why = run(blob + b"\x00")
    assert st == BZK_E_ARG and "after the last record" in why, why
    tag_at = len(recs[0]) + 133 + 8 + 23                                                 # record 1: payment.contract_id behind the 23-byte memo
    assert blob[tag_at:tag_at + 4] == struct.pack("<I", 1)
    st, why = run(blob[:tag_at] + struct.pack("<I", 3) + blob[tag_at + 4:])
    assert st == BZK_E_ARG and "ContractId" in why and "record 1" in why, why
    l1_at = 133 + 8 + 4 + 4 + 32                                                         # record 0: the L1 key's length
    assert blob[l1_at:l1_at + 8] == struct.pack("<Q", 32)
    st, why = run(blob[:l1_at] + struct.pack("<Q", 31) + blob[l1_at + 8:])
    assert st == BZK_E_ARG and "ed25519 public key length" in why and "record 0" in why, why
    bad_bool = blob[:32] + b"\x02" + blob[33:]
    st, why = run(bad_bool)
    assert st == BZK_E_ARG and "bool" in why and "record 0" in why, why
    assert run(blob, 4)[0] == BZK_E_ARG and run(blob, 2)[0] == BZK_E_ARG                  # a count the bytes do not hold
    # the longest payment taken is 65 536 bytes: memo of 65 536 - 112, one byte more is refused
    fits = Wd.signed_withdraw(b"long", 1, "L" * (65536 - 112), Wd.ZIESHA, Wd.ZIESHA, 5, Wd.ZIESHA, 1, hasher=Wd._host_hash)
    over = Wd.signed_withdraw(b"long", 1, "L" * (65537 - 112), Wd.ZIESHA, Wd.ZIESHA, 5, Wd.ZIESHA, 1, hasher=Wd._host_hash)
    assert len(Wd.payment_bytes(fits)) == 65536 and len(Wd.payment_bytes(over)) == 65537
    assert L.host_mpn_withdraw_verify_batch(recs[0] + Wd.enc(fits), 2) == (b"\x03\x03", Wd.fixed_list()[0][3] + Wd.oracle_withdraw(fits, Wd._host_hash)[1])
    st, why = run(recs[0] + Wd.enc(over), 2)
    assert st == BZK_E_ARG and "65536" in why and "record 1" in why, why
    assert run(blob)[0] == BZK_OK and ok.raw == b"\x03\x03\x03"
    assert lib.bzk_mpn_withdraw_verify_batch(None, None, 0, 0, None, None) == BZK_OK
    assert lib.bzk_mpn_withdraw_verify_batch(None, None, 0, 1, ok, None) == BZK_E_ARG
    assert lib.bzk_mpn_withdraw_verify_batch(None, blob, len(blob), n, None, None) == BZK_E_ARG
    w = Wd.admission_world()
    acc = C.c_uint64(99)
    assert lib.bzk_mpn_push_withdraws(w.h, bad_bool, len(bad_bool), n, ok, C.byref(acc)) == BZK_E_ARG and acc.value == 0
    assert lib.bzk_mpn_push_withdraws(None, blob, len(blob), n, ok, None) == BZK_E_ARG
    with pytest.raises(L.BzkError, match="bool"):
        w.push_withdraws(bad_bool, n)
    over_blob = recs[0] + Wd.enc(over)
    assert lib.bzk_mpn_push_withdraws(w.h, over_blob, len(over_blob), 2, ok, C.byref(acc)) == BZK_E_ARG and acc.value == 0


# ---- admission on the host: world B fed wire records against world A fed through bzk_mpn_push_withdraw(fingerprint = NULL)
def test_host_admission_equals_push_withdraw_and_marks_exactly_the_bad_ones():
    want_blob, want_root, good = Wd.world_a()
    assert all(r["payment"]["contract_id"] == Wd.custom(Wd.MPN_CONTRACT) for r in good)
    clean = Wd.admission_world()
    assert Wd.admit(clean, good) == (b"\x01" * len(good), len(good))
    assert clean.make_work(1, sc.VKS, 10, log4_batches=(1, 2, 1)).encode() == want_blob and clean.root() == want_root
    bad = Wd.bad_withdrawals(good)
    verdicts = L.host_mpn_withdraw_verify_batch(b"".join(Wd.enc(r) for _, r in bad), len(bad))[0]
    assert verdicts == b"\x02\x01\x03\x03"  # the last two are refused on contract id / circuit id alone
    mixed = good[:1] + [bad[0][1]] + good[1:3] + [bad[1][1], bad[2][1]] + good[3:] + [bad[3][1]]
    dirty = Wd.admission_world()
    dirty.set_threads(3)
    ok, accepted = Wd.admit(dirty, mixed)
    assert ok == bytes(0 if any(r is b for _, b in bad) else 1 for r in mixed) and accepted == len(good)
    dwork = dirty.make_work(1, sc.VKS, 10, log4_batches=(1, 2, 1))
    assert dwork.encode() == want_blob and dirty.root() == want_root
    r = L.MpnWork.decode(dwork.encode()).synthesize(PROVER)
    assert r.satisfied and (r.accepted, r.rejected) == (len(good), 0)
    assert Wd.admit(dirty, []) == (b"", 0)
    # the records travel: what was admitted is what the work carries
    kind, transitions = B.decode(B.MpnWork, dwork.encode())["data"]
    assert kind == "Withdraw" and [t["tx"] for t in transitions if t["enabled"]] == good
