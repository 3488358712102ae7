"""The wire-form withdrawal producer (bazuka_amd/csrc/bzk_withdraw_sign.cuh, withdraw_sign.hip: bzk_mpn_withdraws_sign) on the CPU.  The
ctx = NULL route - the per-lane function withdraw_sign_one on host threads - is held byte for byte against the records oracle/pyref.py signs
(tests/withdraw_sign_cases.py), against the verify entry and against admission.  tests/host/withdraw_sign_check.hip runs the same per-lane
function and the scatter under the address and undefined-behaviour sanitizers with the field's bound assertions on, over records that lie at
every byte alignment at the end of their heap block."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import r1cs_scenarios as sc
import withdraw_cases as W
import withdraw_sign_cases as K
from bazuka_amd import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(HERE, "host", "_withdraw_sign_check")
NAME = "bzk_mpn_withdraws_sign"
BZK_OK, BZK_E_ARG = 0, -1


def _want(rows):
    return b"".join(W.enc(r[2]) for r in rows), b"".join(W.F(W.fingerprint(r[0])) for r in rows)


def test_name_on_every_surface():
    header = open(os.path.join(ROOT, "include", "bzk.h")).read()
    sys_rs = open(os.path.join(ROOT, "rust", "bzk-sys", "src", "lib.rs")).read()
    shim = open(os.path.join(ROOT, "rust", "bazuka-gpu", "src", "lib.rs")).read()
    lib = L.load_library()
    assert re.search(r"\b%s\(" % NAME, header)
    assert NAME in L.SIGNATURES and getattr(lib, NAME) is not None
    assert L.SIGNATURES[NAME] == L.SIGNATURES["bzk_mpn_txs_sign"]
    assert re.search(r"pub fn %s\(" % NAME, sys_rs)
    assert "sys::%s(" % NAME in shim and "pub fn mpn_withdraws_sign(&self, keys: &[PrivateKey], txs: &mut [MpnWithdraw])" in shim
    assert (L.MPN_TX_CHUNK, L.MPN_WD_CHUNK_BYTES) == (1 << 16, 64 << 20)
    wire = open(os.path.join(ROOT, "bazuka_amd", "csrc", "bzk_mpn_wire.h")).read()
    assert "MPN_TX_CHUNK = (uint64_t)1 << 16" in wire and "MPN_WD_CHUNK_BYTES = (uint64_t)64 << 20" in wire


def test_fixed_list_comes_back_as_pyref_signs_it():
    rows = K.fixed()
    keys, blob, n = K.batch(rows)
    want, want_fp = _want(rows)
    assert all(r[0]["mpn_sig"]["s"] in K.JUNK and r[0]["payment"]["calldata"] in K.JUNK for r in rows)
    assert len({r[0]["mpn_sig"]["s"] for r in rows}) == 2                                     # both kinds of junk occur
    out, ok, fp = L.host_mpn_withdraws_sign(keys, blob, n)
    assert ok == b"\x01" * n
    assert fp == want_fp
    assert out == want
    assert len(out) == len(blob) and out != blob
    assert L.host_mpn_withdraws_sign(keys, blob, n, want_fingerprint=False) == (want, ok, None)
    assert L.host_mpn_withdraw_verify_batch(out, n) == (b"\x03" * n, want_fp)
    # whatever the ignored fields hold, the output is the same: zeros, and the finished record itself
    zeros = b"".join(W.enc(K.blanked(r[2], bytes(32))) for r in rows)
    assert L.host_mpn_withdraws_sign(keys, zeros, n) == (want, ok, want_fp)
    assert L.host_mpn_withdraws_sign(keys, want, n) == (want, ok, want_fp)
    # one record alone, and the list backwards: a record's bytes do not depend on its neighbours
    for i in (0, 4, 8):
        assert L.host_mpn_withdraws_sign(keys[128 * i:128 * i + 128], W.enc(rows[i][0]), 1)[0] == W.enc(rows[i][2])
    back = rows[::-1]
    assert L.host_mpn_withdraws_sign(*K.batch(back))[0] == _want(back)[0]


def test_refusals_are_verdicts_and_leave_record_and_neighbours_alone():
    good = K.fixed()
    for what, rec, key in K.refusals():
        rows = [good[0], (rec, key), good[4]]
        keys, blob, n = K.batch(rows)
        out, ok, fp = L.host_mpn_withdraws_sign(keys, blob, n)
        assert ok == b"\x01\x00\x01", what
        assert out == W.enc(good[0][2]) + W.enc(rec) + W.enc(good[4][2]), what
        assert fp == b"".join(W.F(W.fingerprint(r[0])) for r in rows), what
    every = [(rec, key) for _, rec, key in K.refusals()]
    keys, blob, n = K.batch(every)
    assert n == 10
    out, ok, fp = L.host_mpn_withdraws_sign(keys, blob, n)
    assert ok == bytes(n) and out == blob and fp == W.F(W.fingerprint(every[0][0])) * n


def test_empty_calls_and_bad_arguments():
    lib = L.load_library()
    rows = K.fixed()[:3]
    keys, blob, n = K.batch(rows)
    assert lib.bzk_mpn_withdraws_sign(None, None, None, 0, 0, None, None, None) == BZK_OK
    assert L.host_mpn_withdraws_sign(b"", b"", 0) == (b"", b"", b"")
    out, ok, fp = (C.create_string_buffer(b"\x07" * k, k) for k in (len(blob) + 8, n, 32 * n))

    def run(b, k=n):
        st = lib.bzk_mpn_withdraws_sign(None, keys, b, len(b), k, out, ok, fp)
        assert st == BZK_OK or (out.raw == b"\x07" * (len(blob) + 8) and ok.raw == b"\x07" * n and fp.raw == b"\x07" * 32 * n)  # nothing written
        return st, lib.bzk_mpn_work_last_error().decode()

    st, why = run(blob[:-1])
    assert st == BZK_E_ARG and "record 2" in why, why                                        # a truncated last record
    st, why = run(blob + b"\x00")
    assert st == BZK_E_ARG and "after the last record" in why, why
    st, why = run(blob[:32] + b"\x02" + blob[33:])
    assert st == BZK_E_ARG and "bool" in why and "record 0" in why, why
    assert run(blob, 4)[0] == BZK_E_ARG and run(blob, 2)[0] == BZK_E_ARG                      # a count the bytes do not hold
    assert lib.bzk_mpn_withdraws_sign(None, None, blob, len(blob), n, out, ok, None) == BZK_E_ARG
    assert lib.bzk_mpn_withdraws_sign(None, keys, None, len(blob), n, out, ok, None) == BZK_E_ARG
    assert lib.bzk_mpn_withdraws_sign(None, keys, blob, len(blob), n, None, ok, None) == BZK_E_ARG
    assert lib.bzk_mpn_withdraws_sign(None, keys, blob, len(blob), n, out, None, None) == BZK_E_ARG
    assert out.raw == b"\x07" * (len(blob) + 8)
    with pytest.raises(L.BzkError, match="record 2"):
        L.host_mpn_withdraws_sign(keys, blob[:-1], n)
    with pytest.raises(L.BzkError, match="128"):
        L.host_mpn_withdraws_sign(keys[:-1], blob, n)
    assert run(blob)[0] == BZK_OK and out.raw[:len(blob)] == _want(rows)[0] and out.raw[len(blob):] == b"\x07" * 8


def test_the_longest_payment_is_signed_and_one_byte_more_is_malformed():
    lib = L.load_library()
    first = K.fixed()[0]
    fits = K.unsigned(b"wd sign long", 3, "L" * (65536 - 112), W.ZIESHA, W.ZIESHA, 5, W.ZIESHA, 1)
    over = K.unsigned(b"wd sign long", 3, "L" * (65537 - 112), W.ZIESHA, W.ZIESHA, 5, W.ZIESHA, 1)
    assert len(W.payment_bytes(fits)) == 65536 and len(W.payment_bytes(over)) == 65537
    key = K.key_of(b"wd sign long")
    rows = [first, (fits, key, K.signed_by_pyref(fits, key))]
    out, ok, fp = L.host_mpn_withdraws_sign(*K.batch(rows))
    assert ok == b"\x01\x01" and (out, fp) == _want(rows)
    keys, blob, n = K.batch([first, (over, key)])
    buf, okb = C.create_string_buffer(len(blob)), C.create_string_buffer(2)
    assert lib.bzk_mpn_withdraws_sign(None, keys, blob, len(blob), n, buf, okb, None) == BZK_E_ARG
    why = lib.bzk_mpn_work_last_error().decode()
    assert "65536" in why and "record 1" in why, why
    assert buf.raw == bytes(len(blob)) and okb.raw == bytes(2)


def test_the_withdrawals_of_a_world_come_back_and_are_admitted():
    want_blob, want_root, good = W.world_a()
    accounts = [acct for acct, _, _ in W.WITHDRAWALS]
    keys = b"".join(K.key_of(b"acct%d" % a) for a in accounts)
    blank = b"".join(W.enc(K.blanked(r, K.JUNK[i % 2])) for i, r in enumerate(good))
    out, ok, fp = L.host_mpn_withdraws_sign(keys, blank, len(good))
    assert ok == b"\x01" * len(good)
    assert out == b"".join(W.enc(r) for r in good)
    fresh = W.admission_world()
    assert fresh.push_withdraws(out, len(good)) == (b"\x01" * len(good), len(good))
    assert fresh.make_work(1, sc.VKS, 10, log4_batches=(1, 2, 1)).encode() == want_blob and fresh.root() == want_root


# ---- the per-lane function and the scatter under the sanitizers
def _run_harness(path):
    assert os.path.exists(EXE), "tests/host/_withdraw_sign_check not built (build() compiles it)"
    p = subprocess.run([EXE, path], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    lines = dict(line.split(" ", 1) for line in p.stdout.splitlines() if " " in line)
    assert "eight alignments ok" in p.stdout
    return bytes.fromhex(lines["ok"]), bytes.fromhex(lines["fp"]), bytes.fromhex(lines["out"])


def test_per_lane_function_and_scatter_under_sanitizers(tmp_path):
    good = K.fixed()
    refused = [(rec, key) for _, rec, key in K.refusals()]
    rows = [good[0], good[1], refused[0], good[4], refused[1], refused[5], good[6], good[8], refused[9]]
    keys, blob, n = K.batch(rows)
    starts = [sum(len(W.enc(r[0])) for r in rows[:i]) for i in range(n)]
    assert len({s % 8 for s in starts}) >= 4                                                  # records start at many alignments inside the blob too
    path = tmp_path / "records.bin"
    path.write_bytes(struct.pack("<Q", n) + keys + struct.pack("<Q", len(blob)) + blob)
    ok, fp, out = _run_harness(str(path))
    assert ok == bytes(1 if len(r) == 3 else 0 for r in rows)
    assert fp == b"".join(W.F(W.fingerprint(r[0])) for r in rows)
    assert out == b"".join(W.enc(r[2] if len(r) == 3 else r[0]) for r in rows)
    assert (out, ok, fp) == L.host_mpn_withdraws_sign(keys, blob, n)
