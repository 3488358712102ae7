"""Key decompression and wire-form transaction admission (bazuka_amd/csrc/bzk_decompress.cuh, bzk_mpn_tx_verify_batch, bzk_mpn_push_txs) on the CPU.
The kernels' per-lane functions - the Fr square root, decompress_one, and the composition decompress -> hash input -> Poseidon -> verify_one - run
through tests/host/decompress_check.hip with the bound assertions of the 29-bit field on (an assertion that fires aborts the process) and are compared
with oracle/pycircuit.py pt_decompress, oracle/pyref.py and the product's host mirror bzk_host_jubjub_decompress.  Then the host path of the two
transaction entries: the parser, the verdicts, and admission against a world fed through bzk_mpn_push_tx.  The device run: tests/test_gpu_decompress.py."""
import ctypes as C
import os
import random
import struct

import pytest

import decompress_cases as D
import r1cs_scenarios as sc
from bazuka_amd import lib as L
from oracle import pyref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
R = pr.R_MOD
BZK_OK, BZK_E_ARG = 0, -1
PROVER = bytes(range(1, 33))


@pytest.fixture(scope="module")
def harness(co):
    lib = C.CDLL(os.path.join(ROOT, "tests", "host", "_decompress_check.so"))
    c8, c6 = co.poseidon_params(8), co.poseidon_params(6)

    class H:
        @staticmethod
        def sqrt(vals: bytes):
            n = len(vals) // 32
            out, ok = C.create_string_buffer(32 * n), C.create_string_buffer(n)
            assert lib.dc_sqrt_batch(vals, C.c_uint64(n), out, ok) == 0
            return out.raw, ok.raw

        @staticmethod
        def decompress(x: bytes, odd: bytes):
            n = len(odd)
            xy, ok = C.create_string_buffer(64 * n), C.create_string_buffer(n)
            assert lib.dc_decompress_batch(x, odd, C.c_uint64(n), xy, ok) == 0
            return xy.raw, ok.raw

        @staticmethod
        def tx_verify(txs):
            """the arrays the device path stages, cut here as the library's parser cuts them"""
            n = len(txs)
            nums = (C.c_uint64 * (3 * n))(*[v for t in txs for v in (t["nonce"], t["amount"], t["fee"])])
            ok, h = C.create_string_buffer(n), C.create_string_buffer(32 * n)
            assert lib.dc_tx_verify(b"".join(t["src"][0] for t in txs), bytes(t["src"][1] for t in txs), b"".join(t["dst"][0] for t in txs),
                                    bytes(t["dst"][1] for t in txs), b"".join(F(t["atok"]) + F(t["ftok"]) for t in txs), nums,
                                    b"".join(t["sig"] for t in txs), C.c_uint64(n), c8, len(c8) // 32, c6, len(c6) // 32, 8, 57, ok, h) == 0
            return ok.raw, h.raw
    return H


def test_fixed_keys_against_the_oracle_and_the_host_mirror(harness):
    cases = D.fixed_keys()
    x, odd = b"".join(c[1] for c in cases), bytes(c[2] for c in cases)
    want = [D.expect(c[1], c[2]) for c in cases]
    by_class = {}
    for c, w in zip(cases, want):
        by_class.setdefault(c[0], []).append(w[1])
    assert by_class == {"key": [1] * 16, "x = 0": [1, 1], "x^2 = -1": [1] * 4, "no root": [0] * 16, "limbs of r": [0, 0], "ff..ff": [0, 0]}
    # x = 0: y = 1 (odd) or -1 = r - 1 (even); x^2 = -1: y = 0 for both oddities
    assert [w[0] for c, w in zip(cases, want) if c[0] == "x = 0"] == [F(0) + F(R - 1), F(0) + F(1)]
    assert all(w[0][32:] == F(0) for c, w in zip(cases, want) if c[0] == "x^2 = -1")
    xy, ok = harness.decompress(x, odd)
    hxy, hok = D.host_decompress_all(x, odd, threads=4)
    for i, (c, w) in enumerate(zip(cases, want)):
        assert (xy[64 * i:64 * i + 64], ok[i]) == w, (i, c[0], "harness")
        assert (hxy[64 * i:64 * i + 64], hok[i]) == w, (i, c[0], "host mirror")
        if w[1]:
            p = (U(w[0][:32]), U(w[0][32:]))
            assert pr.jj_on_curve(p) and (p[1] == 0 or p[1] & 1 == c[2]) and w[0][:32] == c[1]


def test_bulk_keys_harness_and_host_mirror_agree_and_accept_by_the_legendre_symbol(harness):
    x, odd = D.bulk_keys(2000, 5)
    xy, ok = harness.decompress(x, odd)
    hxy, hok = D.host_decompress_all(x, odd)
    assert (xy, ok) == (hxy, hok)
    want = bytes(1 if D.is_square(D.radicand(U(x[32 * i:32 * i + 32]))) else 0 for i in range(2000))
    assert ok == want and 800 < sum(want) < 1200
    for i in range(0, 2000, 40):  # a sample of the values themselves against the oracle
        assert (xy[64 * i:64 * i + 64], ok[i]) == D.expect(x[32 * i:32 * i + 32], odd[i])


def test_square_root_alone(harness):
    rnd = random.Random(9)
    vals = [0, 1, 4, R - 1, 7] + [rnd.randrange(R) for _ in range(495)]
    out, ok = harness.sqrt(b"".join(F(v) for v in vals))
    for i, v in enumerate(vals):
        assert ok[i] == (1 if D.is_square(v) else 0), i
        if ok[i]:
            assert pow(U(out[32 * i:32 * i + 32]), 2, R) == v, i
    assert out[:32] == F(0) and ok[:5] == bytes([1, 1, 1, 1 if D.is_square(R - 1) else 0, 0])  # 7 is a non-residue
    assert 200 < sum(ok) < 300


def test_host_decompress_refuses_null_pointers():
    lib, b = L.load_library(), C.create_string_buffer(64)
    assert lib.bzk_host_jubjub_decompress(None, 0, b) == BZK_E_ARG and lib.bzk_host_jubjub_decompress(b, 0, None) == BZK_E_ARG


# ---- transactions
def test_encoder_gives_the_record_lengths_of_the_wire_format():
    lens = {len(D.enc_tx(t)) for _, t, _, _ in D.tx_list()}
    assert lens == {190, 222, 254}


def test_transaction_list_on_the_harness_and_the_host_entry(harness):
    cases = D.tx_list()
    assert len(cases) == 8 + 4 * len(D.MUTATIONS)
    want_ok, want_h = bytes(c[2] for c in cases), b"".join(c[3] for c in cases)
    by = {k: [c[2] for c in cases if c[0] == k] for k in ("valid",) + D.MUTATIONS}
    assert by["valid"] == [1] * 8 and all(by[k] == [0] * 4 for k in D.MUTATIONS), by
    assert all(c[3] == bytes(32) for c in cases if c[0] == "dst.x without a root")
    # a flipped dst oddity changes the message (dst.y enters the hash), a flipped src oddity does not
    for k in range(4):
        base, flipped_src, flipped_dst = cases[k], cases[8 + k * len(D.MUTATIONS)], cases[8 + k * len(D.MUTATIONS) + 1]
        assert flipped_src[3] == base[3] and flipped_dst[3] != base[3]
    ok, h = harness.tx_verify([c[1] for c in cases])
    assert ok == want_ok, [(i, c[0]) for i, c in enumerate(cases) if ok[i] != c[2]]
    assert h == want_h
    blob = b"".join(D.enc_tx(c[1]) for c in cases)
    assert L.host_mpn_tx_verify_batch(blob, len(cases)) == (want_ok, want_h)
    assert L.host_mpn_tx_verify_batch(blob, len(cases), want_hash=False) == (want_ok, None)


def test_scalars_that_are_not_residues_are_verdicts_not_errors(harness):
    t = D.tx_list()[0][1]  # a Custom amount token: the record carries its 32 bytes
    blob = D.enc_tx(t)
    txs = []
    for off in (4, 37, 74, 126, 158, 190):  # src.x, dst.x, the Custom token id, r.x, r.y, s
        txs.append(blob[:off] + D.R_LIMBS + blob[off + 32:])
        txs.append(blob[:off] + D.ALL_ONES + blob[off + 32:])
    ok, h = L.host_mpn_tx_verify_batch(blob + b"".join(txs), 1 + len(txs))
    assert ok == b"\x01" + bytes(len(txs))
    assert h[:32] == D.oracle_tx(t)[1] and h[32 + 64:32 + 192] == bytes(128)  # dst.x, token id: nothing to hash


def test_malformed_records_are_refused():
    lib = L.load_library()
    cases = D.tx_list()
    blob = b"".join(D.enc_tx(c[1]) for c in cases[:3])
    n = 3
    ok = C.create_string_buffer(n)

    def run(b, k=n):
        st = lib.bzk_mpn_tx_verify_batch(None, b, len(b), k, ok, None)
        return st, lib.bzk_mpn_work_last_error().decode()

    assert run(blob)[0] == BZK_OK
    st, why = run(blob[:-1])
    assert st == BZK_E_ARG and "record 2" in why, why                                    # a truncated last record
    st, why = run(blob + b"\x00")
    assert st == BZK_E_ARG and "after the last record" in why, why
    first = len(D.enc_tx(cases[0][1]))
    bad_tag = blob[:70] + struct.pack("<I", 3) + blob[74:]                               # record 0: amount ContractId tag
    assert blob[70:74] == struct.pack("<I", 2)
    st, why = run(bad_tag)
    assert st == BZK_E_ARG and "ContractId" in why and "record 0" in why, why
    bad_bool = blob[:first + 36] + b"\x02" + blob[first + 37:]                           # record 1: src oddity
    st, why = run(bad_bool)
    assert st == BZK_E_ARG and "bool" in why and "record 1" in why, why
    assert run(blob, 4)[0] == BZK_E_ARG and run(blob, 2)[0] == BZK_E_ARG                  # a count the bytes do not hold
    assert lib.bzk_mpn_tx_verify_batch(None, None, 0, 0, None, None) == BZK_OK
    assert lib.bzk_mpn_tx_verify_batch(None, None, 0, 1, ok, None) == BZK_E_ARG and lib.bzk_mpn_tx_verify_batch(None, blob, len(blob), n, None, None) == BZK_E_ARG
    w = L.MpnWorld(3, 3)
    acc = C.c_uint64(99)
    assert lib.bzk_mpn_push_txs(w.h, bad_bool, len(bad_bool), n, ok, C.byref(acc)) == BZK_E_ARG and acc.value == 0
    assert lib.bzk_mpn_push_txs(None, blob, len(blob), n, ok, None) == BZK_E_ARG
    with pytest.raises(L.BzkError, match="bool"):
        w.push_txs(bad_bool, n)


# ---- admission on the host: a world fed wire-form transactions against a twin fed through bzk_mpn_push_tx
def test_host_admission_equals_push_tx_and_marks_exactly_the_bad_ones():
    good = D.wire_transfers()
    want, want_root = D.twin_work()
    clean = D.admission_world()
    assert D.admit(clean, good) == (b"\x01" * len(good), len(good))
    work = clean.make_work(2, sc.VKS, 10, log4_batches=(1, 1, 2))
    assert work.encode() == want.encode() and clean.root() == want_root
    # three bad ones interleaved: marked, not queued, and the work is the twin's that never saw them
    bad = D.bad_transfers(good)
    mixed = good[:2] + [bad[0]] + good[2:5] + [bad[1]] + good[5:] + [bad[2]]
    dirty = D.admission_world()
    dirty.set_threads(3)
    ok, accepted = D.admit(dirty, mixed)
    assert ok == bytes(0 if any(t is b for b in bad) else 1 for t in mixed) and accepted == len(good)
    dwork = dirty.make_work(2, sc.VKS, 10, log4_batches=(1, 1, 2))
    assert dwork.encode() == want.encode() and dirty.root() == want_root
    r = L.MpnWork.decode(dwork.encode()).synthesize(PROVER)
    assert r.satisfied and (r.accepted, r.rejected) == (len(good), 0)
    rt = L.MpnWork.decode(want.encode()).synthesize(PROVER)
    assert (rt.accepted, rt.rejected) == (r.accepted, r.rejected) and rt.view("z") == r.view("z")
    assert D.admit(dirty, []) == (b"", 0)
