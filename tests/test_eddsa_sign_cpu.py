"""Batched key derivation and signing (bazuka_amd/csrc/bzk_eddsa_sign.cuh, sign.hip: bzk_jubjub_keys_batch, bzk_jubjub_sign_batch, bzk_mpn_txs_sign)
on the CPU.  tests/host/eddsa_sign_check.hip runs the per-lane functions under the address and undefined-behaviour sanitizers with the field's
bound assertions on: the reduction modulo the subgroup order on a table of operands (re-computed here with Python integers) and the reference
fixture.  The ctx = NULL route of the entry points - the same per-lane functions on host threads - is held against the host single calls
(bzk_host_jubjub_sign, bzk_host_jubjub_keys, bzk_host_jubjub_verify), oracle/pyref.py (jj_sign, jj_generate_keys) and decompress_cases.signed_tx."""
import ctypes as C
import json
import os
import random
import struct
import subprocess

import decompress_cases as D
import sign_cases as S
from bazuka_amd import lib as L
from oracle import pyref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "host", "_eddsa_sign_check")
REF = json.load(open(os.path.join(HERE, "golden", "reference_vectors.json")))
F, U = S.F, S.U
R, ORDER = S.R, S.ORDER
BZK_OK, BZK_E_ARG = 0, -1
SET = (0, 1, ORDER - 1, ORDER, ORDER + 1, 1 << 252, 1 << 254, R - 1)


def _run(args):
    assert os.path.exists(EXE), "tests/host/_eddsa_sign_check not built (build() compiles it)"
    p = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return p.stdout


def test_per_lane_functions_under_sanitizers():
    j = REF["jubjub_abc"]
    out = _run(j["pub"] + j["sig_r"] + [j["sig_s"], hex(j["message"])])
    assert "rows ok" in out and "fixture ok" in out, out


def test_reduction_table_is_what_python_integers_give():
    rows = [tuple(int(v, 16) for v in line.split()) for line in _run(["--dump"]).splitlines()]
    assert all(max(h, a, r) < R and want == (h * a + r) % ORDER for h, a, r, want in rows)
    have = {(h, a, r) for h, a, r, _ in rows}
    assert all((h, a, r) in have for h in SET for a in SET for r in SET)                    # every operand at every value of the set
    off_grid = [(h, a, r) for h, a, r, _ in rows if not (h in SET and a in SET and r in SET)]
    assert sum((h * a + r) % ORDER == 0 for h, a, r in off_grid) >= 8                        # exact multiples of ORDER
    assert sum((h * a + r) % ORDER == ORDER - 1 for h, a, r in off_grid) >= 8               # one below an exact multiple
    assert any((h * a + r) >> 509 for h, a, r in off_grid)                                   # and the widest sums


def _sign_host_rows(keys, msgs):
    n = len(msgs) // 32
    return b"".join(L.host_jubjub_sign(keys[128 * i:128 * i + 128], msgs[32 * i:32 * i + 32]) for i in range(n))


def test_sign_batch_equals_the_host_signer_row_by_row():
    for n in (1, 63, 64, 65, 257):
        keys, msgs = S.rows(n, 9000 + n)
        sig, ok = L.host_jubjub_sign_batch(keys, msgs)
        assert ok == b"\x01" * n
        assert sig == _sign_host_rows(keys, msgs), n
        assert all(L.host_jubjub_verify(keys[128 * i:128 * i + 64], msgs[32 * i:32 * i + 32], sig[96 * i:96 * i + 96]) for i in range(n))


def test_sign_batch_equals_pyref_on_sixteen_rows():
    keys, msgs = S.rows(16, 9100)
    sig, ok = L.host_jubjub_sign_batch(keys, msgs)
    assert ok == b"\x01" * 16
    for i in range(16):
        want = pr.jj_sign(S.key_dict(keys[128 * i:128 * i + 128]), U(msgs[32 * i:32 * i + 32]))
        assert sig[96 * i:96 * i + 96] == S.sig_bytes(want), i


def test_keys_batch_at_the_rate_boundary():
    seeds = S.seeds()
    assert tuple(len(s) for s in seeds) == S.SEED_LENGTHS
    keys = L.host_jubjub_keys_batch(seeds)
    for i, s in enumerate(seeds):
        got = keys[128 * i:128 * i + 128]
        assert got == L.host_jubjub_keys(s), len(s)
        assert got == S.key_bytes(pr.jj_generate_keys(s)), len(s)
    assert L.host_jubjub_keys_batch([b"", b""]) == keys[:128] * 2                             # no seed bytes at all
    assert L.host_jubjub_keys_batch([]) == b""


def test_crafted_key_rows_equal_pyref():
    cases = S.crafted()
    keys, msgs = b"".join(c[1] for c in cases), b"".join(c[2] for c in cases)
    sig, ok = L.host_jubjub_sign_batch(keys, msgs)
    assert ok == b"\x01" * len(cases)
    for i, c in enumerate(cases):
        assert sig[96 * i:96 * i + 96] == c[3], c[0]
    assert sig == _sign_host_rows(keys, msgs)                                                # the host signer takes the same rows the same way


def test_a_non_residue_in_any_field_is_a_verdict_and_leaves_its_neighbours_alone():
    keys, msgs = S.rows(3, 9200)
    good = _sign_host_rows(keys, msgs)
    for field, key, msg in S.non_residue_rows():
        k = keys[:128] + key + keys[128:]
        m = msgs[:32] + msg + msgs[32:]
        sig, ok = L.host_jubjub_sign_batch(k, m)
        assert ok == b"\x01\x00\x01\x01", field
        assert sig == good[:96] + bytes(96) + good[96:], field


def test_interleaved_rows_are_consistent():
    keys, msgs, want_ok, want_sig = S.interleaved(65, 9300)
    sig, ok = L.host_jubjub_sign_batch(keys, msgs)
    assert ok == want_ok and 0 in want_ok and len(want_sig) == len(S.crafted())
    for i, w in want_sig.items():
        assert sig[96 * i:96 * i + 96] == w
    assert all(sig[96 * i:96 * i + 96] == bytes(96) for i in range(len(ok)) if not ok[i])


def test_empty_calls_and_bad_arguments():
    lib = L.load_library()
    buf = C.create_string_buffer(256)
    off = (C.c_uint64 * 2)(0, 3)
    assert lib.bzk_jubjub_sign_batch(None, None, None, 0, None, None) == BZK_OK
    assert lib.bzk_jubjub_keys_batch(None, None, None, 0, None) == BZK_OK
    assert lib.bzk_mpn_txs_sign(None, None, None, 0, 0, None, None, None) == BZK_OK
    assert lib.bzk_jubjub_sign_batch(None, None, buf, 1, buf, buf) == BZK_E_ARG and lib.bzk_jubjub_sign_batch(None, buf, buf, 1, buf, None) == BZK_E_ARG
    assert lib.bzk_jubjub_keys_batch(None, None, off, 1, buf) == BZK_E_ARG                   # three seed bytes and no pointer to them
    bad = (C.c_uint64 * 3)(0, 3, 2)
    assert lib.bzk_jubjub_keys_batch(None, b"abc", bad, 2, buf) == BZK_E_ARG                 # offsets that go back
    assert lib.bzk_jubjub_sign_batch_dev(None, buf, buf, 1, buf, buf) == BZK_E_ARG and lib.bzk_jubjub_keys_batch_dev(None, buf, off, 1, buf) == BZK_E_ARG


# ---- bzk_mpn_txs_sign
def test_txs_sign_reproduces_signed_tx_on_the_eight_token_pair_forms():
    base = [c[1] for c in D.tx_list()[:8]]
    assert sorted({len(D.enc_tx(t)) for t in base}) == [190, 222, 254]
    keys = b"".join(L.host_jubjub_keys(b"tx src %d" % k) for k in range(8))
    blank = b"".join(D.enc_tx(dict(t, sig=bytes([0xA5]) * 96)) for t in base)                 # the input's signature bytes are ignored
    out, ok, h = L.host_mpn_txs_sign(keys, blank, 8)
    assert ok == b"\x01" * 8
    assert out == b"".join(D.enc_tx(t) for t in base)
    assert h == b"".join(c[3] for c in D.tx_list()[:8])
    assert L.host_mpn_tx_verify_batch(out, 8) == (b"\x01" * 8, h)
    assert L.host_mpn_txs_sign(keys, blank, 8, want_hash=False) == (out, ok, None)


def test_txs_sign_leaves_a_record_it_cannot_sign_unchanged():
    rnd = random.Random(5)
    base = [c[1] for c in D.tx_list()[:4]]
    keys = b"".join(L.host_jubjub_keys(b"tx src %d" % k) for k in range(4))
    stamp = bytes([0x5A]) * 96
    txs = [dict(base[0], sig=stamp), dict(D.mutate(base[1], "dst.x without a root", rnd), sig=stamp), dict(D.mutate(base[2], "src oddity", rnd), sig=stamp),
           dict(base[3], sig=stamp)]
    blob = b"".join(D.enc_tx(t) for t in txs)
    out, ok, h = L.host_mpn_txs_sign(keys, blob, 4)
    assert ok == b"\x01\x00\x00\x01"
    want = [D.enc_tx(base[0]), D.enc_tx(txs[1]), D.enc_tx(txs[2]), D.enc_tx(base[3])]
    assert out == b"".join(want)
    assert h[32:64] == bytes(32) and h[64:96] == D.oracle_tx(base[2])[1]                      # no dst, no hash; a src that is not the key's still hashes
    # a key that belongs to another record, and a key with a non-residue: verdicts, records unchanged
    swapped = keys[128:256] + keys[:128] + keys[256:]
    out2, ok2, _ = L.host_mpn_txs_sign(swapped, blob, 4)
    assert ok2 == b"\x00\x00\x00\x01" and out2 == b"".join([D.enc_tx(txs[0])] + want[1:])
    for f in range(4):
        broken = keys[:32 * f] + D.R_LIMBS + keys[32 * f + 32:]
        out3, ok3, _ = L.host_mpn_txs_sign(broken, blob, 4)
        assert ok3 == b"\x00\x00\x00\x01" and out3 == out2, f


def test_txs_sign_refuses_malformed_buffers():
    lib = L.load_library()
    base = [c[1] for c in D.tx_list()[:3]]
    keys = b"".join(L.host_jubjub_keys(b"tx src %d" % k) for k in range(3))
    blob = b"".join(D.enc_tx(t) for t in base)
    out, ok = C.create_string_buffer(len(blob) + 8), C.create_string_buffer(3)

    def run(b, k=3):
        st = lib.bzk_mpn_txs_sign(None, keys, b, len(b), k, out, ok, None)
        return st, lib.bzk_mpn_work_last_error().decode()

    assert run(blob)[0] == BZK_OK
    st, why = run(blob[:-1])
    assert st == BZK_E_ARG and "record 2" in why, why                                        # a truncated last record
    assert blob[70:74] == struct.pack("<I", 2)
    st, why = run(blob[:70] + struct.pack("<I", 3) + blob[74:])                              # record 0: a raised ContractId tag
    assert st == BZK_E_ARG and "ContractId" in why and "record 0" in why, why
    first = len(D.enc_tx(base[0]))
    st, why = run(blob[:first + 36] + b"\x02" + blob[first + 37:])                           # record 1: a raised oddity byte
    assert st == BZK_E_ARG and "bool" in why and "record 1" in why, why
    assert run(blob, 4)[0] == BZK_E_ARG and run(blob, 2)[0] == BZK_E_ARG                      # a count the bytes do not hold
    assert lib.bzk_mpn_txs_sign(None, None, blob, len(blob), 3, out, ok, None) == BZK_E_ARG
    assert lib.bzk_mpn_txs_sign(None, keys, blob, len(blob), 3, None, ok, None) == BZK_E_ARG
