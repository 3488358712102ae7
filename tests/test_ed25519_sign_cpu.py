"""Ed25519 key derivation and signing (bazuka_amd/csrc/bzk_ed25519_sign.cuh, ed_sign.hip, wire.hip: bzk_host_ed25519_keys / _sign,
bzk_ed25519_keys_batch, bzk_ed25519_sign_batch, bzk_mpn_deposits_sign, bzk_l1_txs_sign) on the CPU: the host single calls and the ctx = NULL route
of the batch entries - the per-lane functions the kernels run, on host threads.  Signing is deterministic, so every byte is pinned: on the
OpenSSL / RFC 8032 fixture tests/golden/ed25519_sign_vectors.json, on the restatement ed25519_cases.sign (Python integers and hashlib) and, for
the wire records, on the records ed25519_cases / l1_tx_cases sign in Python.  tests/host/ed25519_sign_check.hip runs sc_muladd and
base_mul_encode under the address and undefined-behaviour sanitizers against tables made here with Python integers."""
import copy
import hashlib
import os
import random
import subprocess

import pytest

import bincode_ref as B
import ed25519_cases as E
import ed25519_sign_cases as S
import l1_tx_cases as T
from bazuka_amd import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "host", "_ed25519_sign_check")
ORDER = E.L_ORDER


def _secret(tag) -> bytes:
    return hashlib.sha256(b"ed25519 sign test %r" % (tag,)).digest()


@pytest.fixture(scope="module")
def fixture():
    return S.fixture()


# ---- the per-lane functions under the sanitizers ---------------------------------------------------------------------------------------------
def _run(mode, rows, tmp_path):
    assert os.path.exists(EXE), "tests/host/_ed25519_sign_check not built (build() compiles it)"
    path = tmp_path / "table.txt"
    path.write_text("".join(" ".join(r) + "\n" for r in rows))
    p = subprocess.run([EXE, mode, str(path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    assert "clamp ok" in p.stdout and "%d rows ok" % len(rows) in p.stdout, p.stdout
    return p.stdout


def test_sc_muladd_against_python_integers(tmp_path):
    rnd = random.Random(252)
    ks = (0, 1, ORDER - 1)
    avals = (0, 8, 1 << 254, (1 << 254) + 8, (1 << 255) - 8, (1 << 256) - 1)
    ops = [(k, a, r) for k in ks for a in avals for r in ks]
    for _ in range(16):  # k a + r an exact multiple of l, and one below one: r = -k a (mod l), or that minus 1, both below l
        k, a = rnd.randrange(1, ORDER), (rnd.randrange(1 << 251) << 3) | (1 << 254)
        ops.append((k, a, (-k * a) % ORDER))
        ops.append((k, a, (-k * a - 1) % ORDER))
    for _ in range(500):
        ops.append((rnd.randrange(ORDER), (rnd.randrange(1 << 251) << 3) | (1 << 254), rnd.randrange(ORDER)))
    assert sum((k * a + r) % ORDER == 0 for k, a, r in ops[54:]) >= 16 and sum((k * a + r) % ORDER == ORDER - 1 for k, a, r in ops[54:]) >= 16
    _run("--muladd", [tuple("%064x" % v for v in (k, a, r, (k * a + r) % ORDER)) for k, a, r in ops], tmp_path)


def test_base_mul_encode_against_python_integers(tmp_path):
    ks = (0, 1, ORDER - 1, ORDER, (1 << 255) - 8, (1 << 256) - 1)
    rows = [("%064x" % k, E.encode(E.mul(k, E.BASE)).hex()) for k in ks]
    assert rows[0][1] == rows[3][1] == (1).to_bytes(32, "little").hex()  # the neutral element's encoding, at 0 and at l
    _run("--encode", rows, tmp_path)


# ---- plain signing and keys ------------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_sweep_and_agrees_with_the_restatement(fixture):
    assert sorted({len(v["msg"]) for v in fixture if "rfc" not in v}) == sorted(S.LENGTHS)
    assert sum(v["openssl"] for v in fixture) >= 2 * (len(S.LENGTHS) - 1) and sum("rfc" in v for v in fixture) == 2
    for v in fixture:
        assert E.public_key(v["secret"]) == v["pk"] and E.sign(v["secret"], v["msg"]) == v["sig"]


def test_host_sign_and_batch_equal_the_fixture(fixture):
    keys = b"".join(v["secret"] + v["pk"] for v in fixture)
    msgs = [v["msg"] for v in fixture]
    want = b"".join(v["sig"] for v in fixture)
    assert b"".join(L.host_ed25519_sign(v["secret"] + v["pk"], v["msg"]) for v in fixture) == want
    assert L.host_ed25519_sign_batch(keys, msgs) == want
    assert L.host_ed25519_sign_batch(b"", []) == b""


def test_length_sweep_equals_the_restatement_and_verifies():
    secret = _secret("sweep")
    key = S.keypair(secret)
    msgs = S.messages(len(S.LENGTHS), 1)
    assert [len(m) for m in msgs] == list(S.LENGTHS)
    sig = L.host_ed25519_sign_batch(key * len(msgs), msgs)
    for i, m in enumerate(msgs):
        s = sig[64 * i:64 * i + 64]
        assert s == E.sign(secret, m) == L.host_ed25519_sign(key, m), len(m)
        assert E.verify(key[32:], m, s) and L.host_ed25519_verify(key[32:], m, s), len(m)
        if m:
            assert not L.host_ed25519_verify(key[32:], T.flip(m, len(m) // 2), s)
    assert L.host_ed25519_verify_batch(key[32:] * len(msgs), msgs, sig) == b"\x01" * len(msgs)


def test_the_public_half_is_taken_as_given():
    """dalek's ExpandedSecretKey::sign(message, &public): another A changes k and s, not R"""
    secret, other = _secret("a"), E.public_key(_secret("b"))
    a, prefix = E._expand(secret)
    m = b"message"
    r = int.from_bytes(E.sha512(prefix + m), "little") % ORDER
    rb = E.encode(E.mul(r, E.BASE))
    k = int.from_bytes(E.sha512(rb + other + m), "little") % ORDER
    assert L.host_ed25519_sign(secret + other, m) == rb + ((r + k * a) % ORDER).to_bytes(32, "little")


def test_keys_equal_the_restatement():
    seeds = S.seeds(12)
    assert [len(s) for s in seeds[:7]] == list(S.SEED_LENGTHS) + [3] and seeds[6] == b"ABC"
    want = b"".join(S.secret_of(s) + E.public_key(S.secret_of(s)) for s in seeds)
    assert b"".join(L.host_ed25519_keys(s) for s in seeds) == want
    assert L.host_ed25519_keys_batch(seeds) == want
    assert all(want[64 * i + 31] < 0x80 for i in range(len(seeds)))
    assert L.host_ed25519_keys_batch([]) == b"" and L.host_ed25519_keys_batch([b"", b""]) == L.host_ed25519_keys(b"") * 2


def test_bad_arguments_are_refused():
    lib = L.load_library()
    off = (L.C.c_uint64 * 3)(0, 5, 3)  # decreasing
    out = L.C.create_string_buffer(128)
    assert lib.bzk_ed25519_sign_batch(None, bytes(128), b"abcde", off, 2, out) == -1
    assert lib.bzk_ed25519_keys_batch(None, b"abcde", off, 2, out) == -1
    off = (L.C.c_uint64 * 3)(1, 2, 3)  # not from 0
    assert lib.bzk_ed25519_sign_batch(None, bytes(128), b"abcde", off, 2, out) == -1
    assert lib.bzk_ed25519_sign_batch(None, None, b"abcde", off, 2, out) == -1
    assert lib.bzk_host_ed25519_sign(None, b"", 0, out) == -1 and lib.bzk_host_ed25519_keys(None, 3, out) == -1


# ---- deposits --------------------------------------------------------------------------------------------------------------------------------
# test_deposit_admit_cpu's padding edges (64 + the unsigned payment at 239, 240, 255, 256, 257) and the same edges of the first hash (32 + ...)
MEMO_LENGTHS = (58, 59, 74, 75, 76, 90, 91, 106, 107, 108)


@pytest.fixture(scope="module")
def deposits():
    secrets = [_secret(("deposit", k)) for k in MEMO_LENGTHS]
    recs = [E.signed_deposit(s, S.ADDRESS, "e" * k, E.ZIESHA, E.ZIESHA, 9, E.ZIESHA, 1) for s, k in zip(secrets, MEMO_LENGTHS)]
    assert {(64 + len(E.unsigned_bytes(r))) % 128 for r in recs[:5]} == {111, 112, 127, 0, 1}
    assert {(32 + len(E.unsigned_bytes(r))) % 128 for r in recs[5:]} == {111, 112, 127, 0, 1}
    return b"".join(S.keypair(s) for s in secrets), recs


def _with_sig(rec, sig):
    return dict(rec, payment=dict(rec["payment"], sig=sig))


@pytest.mark.parametrize("prefixed", [False, True])
def test_deposits_come_back_as_python_signs_them(deposits, prefixed):
    keys, recs = deposits
    n = len(recs)
    want = b"".join(E.enc(r, prefixed) for r in recs)
    L.mpn_set_wire_flags(1 if prefixed else 0)
    try:
        for sig in (None, bytes(range(64))):  # None, and a garbage Some
            blob = b"".join(E.enc(_with_sig(r, sig), prefixed) for r in recs)
            got_sig, ok, out = L.host_mpn_deposits_sign(keys, blob, n)
            assert ok == b"\x01" * n and out == want
            assert got_sig == b"".join(r["payment"]["sig"] for r in recs)
            assert L.host_mpn_deposits_sign(keys, blob, n, want_txs=False) == (got_sig, ok, None)
        assert all(v & 1 for v in L.host_mpn_deposit_verify_batch(want, n, want_address=False)[0])  # bit 0: payment.verify_signature()
    finally:
        L.mpn_set_wire_flags(0)


def test_a_deposit_of_another_key_is_left_alone(deposits):
    keys, recs = deposits
    n = len(recs)
    blob_recs = [E.enc(_with_sig(r, None if i % 2 else bytes(64))) for i, r in enumerate(recs)]
    wrong = bytearray(keys)
    wrong[64 * 3:64 * 4], wrong[64 * 4:64 * 5] = keys[64 * 4:64 * 5], keys[64 * 3:64 * 4]  # records 3 and 4 get each other's key
    sig, ok, out = L.host_mpn_deposits_sign(bytes(wrong), b"".join(blob_recs), n)
    assert ok == bytes(0 if i in (3, 4) else 1 for i in range(n))
    assert sig[64 * 3:64 * 5] == bytes(128)
    assert out == b"".join(blob_recs[i] if i in (3, 4) else E.enc(r) for i, r in enumerate(recs))


def test_deposit_cap_out_len_and_refusals(deposits):
    keys, recs = deposits
    n = len(recs)
    lib = L.load_library()
    blob = b"".join(E.enc(_with_sig(r, None)) for r in recs)
    want = b"".join(E.enc(r) for r in recs)
    sig, ok = L.C.create_string_buffer(b"\x07" * 64 * n, 64 * n), L.C.create_string_buffer(b"\x07" * n, n)
    out, out_len = L.C.create_string_buffer(b"\x07" * len(want), len(want)), L.C.c_uint64(0)
    st = lib.bzk_mpn_deposits_sign(None, keys, blob, len(blob), n, sig, ok, out, len(want) - 1, L.C.byref(out_len))
    assert st == -1 and out_len.value == len(want) == len(blob) + 64 * n
    assert sig.raw == b"\x07" * 64 * n and ok.raw == b"\x07" * n and out.raw == b"\x07" * len(want)  # nothing written
    st = lib.bzk_mpn_deposits_sign(None, keys, blob, len(blob), n, sig, ok, out, len(want), L.C.byref(out_len))
    assert st == 0 and out.raw == want and out_len.value == len(want)
    out_len = L.C.c_uint64(0)
    st = lib.bzk_mpn_deposits_sign(None, keys, blob, len(blob), n, sig, ok, None, 0, L.C.byref(out_len))  # txs_out NULL: only sig and ok
    assert st == 0 and out_len.value == len(want) and sig.raw == b"".join(r["payment"]["sig"] for r in recs)
    with pytest.raises(L.BzkError, match="record %d" % (n - 1)):
        L.host_mpn_deposits_sign(keys, blob[:-1], n)
    with pytest.raises(L.BzkError) as e_sign:
        L.host_mpn_deposits_sign(keys, blob + b"\0", n)
    with pytest.raises(L.BzkError) as e_verify:
        L.host_mpn_deposit_verify_batch(blob + b"\0", n)
    assert str(e_sign.value).split("[")[1] == str(e_verify.value).split("[")[1]  # the verify entry's refusal, word for word
    assert L.host_mpn_deposits_sign(b"", b"", 0) == (b"", b"", b"")


# ---- L1 transactions -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def l1_rows():
    """(secrets, transactions signed in Python) for the seven variants, the memo sweep and the cut sweep, each re-signed by a 32-byte secret of
    its own row (the corpora's own wallets are strings of other lengths, which a 64-byte key row cannot carry)"""
    txs = [copy.deepcopy(t) for t in T.variant_txs()]
    txs += [B.decode(T.schema(T.FORM_TX), r) for r in T.memo_sweep()]
    txs += [B.decode(T.schema(T.FORM_TX), r) for r in T.cut_sweep()]
    secrets = [_secret(("l1", i % 5)) for i in range(len(txs))]
    return secrets, [T.sign_tx(s, t) for s, t in zip(secrets, txs)]


@pytest.mark.parametrize("form", [T.FORM_TX, T.FORM_TX_AND_DELTA])
def test_l1_records_come_back_as_python_signs_them(l1_rows, form):
    secrets, txs = l1_rows
    n = len(txs)
    pub = {s: E.public_key(s) for s in set(secrets)}
    keys = b"".join(s + pub[s] for s in secrets)
    sd = [T.delta_pairs(i % 3) if form == T.FORM_TX_AND_DELTA and i % 4 else None for i in range(n)]
    want = [T.enc(t, form, False, d) for t, d in zip(txs, sd)]
    blob = b"".join(T.enc(dict(t, sig=("Unsigned", None)), form, False, d) for t, d in zip(txs, sd))
    sig, ok, h, out = L.host_l1_txs_sign(keys, blob, n, form)
    assert ok == b"\x01" * n
    assert sig == b"".join(t["sig"][1] for t in txs)
    assert out == b"".join(want)
    assert h == b"".join(hashlib.sha3_256(T.signed_bytes(t)).digest() for t in txs)
    assert h[:32 * 7] == b"".join(T.expected(r, form)[1] for r in want[:7])
    ok_v, h_v = L.host_l1_tx_verify_batch(out, n, form)
    assert ok_v == b"\x01" * n and h_v == h
    # Signed input (its bytes ignored), and without hashes or records
    garbled = b"".join(T.enc(dict(t, sig=("Signed", bytes(range(64)))), form, False, d) for t, d in zip(txs[:16], sd))
    assert L.host_l1_txs_sign(keys[:64 * 16], garbled, 16, form, want_hash=False, want_txs=False) == (sig[:64 * 16], ok[:16], None, None)
    assert L.host_l1_txs_sign(keys[:64 * 16], garbled, 16, form)[3] == b"".join(want[:16])


def test_l1_length_prefixed_signatures_follow_the_wire_flag():
    secrets = [_secret(("l1p", i)) for i in range(7)]
    txs = [T.sign_tx(s, copy.deepcopy(t), True) for s, t in zip(secrets, T.variant_txs(True))]
    keys = b"".join(S.keypair(s) for s in secrets)
    L.mpn_set_wire_flags(1)
    try:
        for form in (T.FORM_TX, T.FORM_TX_AND_DELTA):
            sd = T.delta_pairs(2) if form == T.FORM_TX_AND_DELTA else None
            blob = b"".join(T.enc(dict(t, sig=("Unsigned", None)), form, True, sd) for t in txs)
            sig, ok, h, out = L.host_l1_txs_sign(keys, blob, 7, form)
            assert ok == b"\x01" * 7 and out == b"".join(T.enc(t, form, True, sd) for t in txs)
            assert len(out) == len(blob) + 72 * 7
    finally:
        L.mpn_set_wire_flags(0)


def test_l1_without_src_or_of_another_key_is_left_alone():
    secrets = [_secret(("l1n", i)) for i in range(7)]
    txs = [T.sign_tx(s, copy.deepcopy(t)) for s, t in zip(secrets, T.variant_txs())]
    keys = b"".join(S.keypair(s) for s in secrets)
    recs = [T.enc(dict(t, sig=("Unsigned", None))) for t in txs]
    recs[2] = T.enc(dict(txs[2], src=None, sig=("Unsigned", None)))
    recs[5] = T.enc(dict(txs[5], src=E.public_key(b"someone else")))  # Signed by the test's wallet, src another key
    sig, ok, h, out = L.host_l1_txs_sign(keys, b"".join(recs), 7)
    assert ok == bytes(0 if i in (2, 5) else 1 for i in range(7))
    assert sig[64 * 2:64 * 3] == bytes(64) and sig[64 * 5:64 * 6] == bytes(64)
    assert out == b"".join(recs[i] if i in (2, 5) else T.enc(t) for i, t in enumerate(txs))
    assert h == b"".join(T.expected(r)[1] for r in recs)
    lib = L.load_library()
    blob, want_len = b"".join(recs), len(out)
    osig, ook, obuf, out_len = L.C.create_string_buffer(64 * 7), L.C.create_string_buffer(7), L.C.create_string_buffer(b"\x07" * want_len, want_len), L.C.c_uint64(0)
    st = lib.bzk_l1_txs_sign(None, keys, blob, len(blob), 7, 0, osig, ook, None, obuf, want_len - 1, L.C.byref(out_len))
    assert st == -1 and out_len.value == want_len and obuf.raw == b"\x07" * want_len and ook.raw == bytes(7)
    with pytest.raises(L.BzkError, match="record 6"):
        L.host_l1_txs_sign(keys, blob[:-1], 7)
    assert lib.bzk_l1_txs_sign(None, keys, blob, len(blob), 7, 2, osig, ook, None, None, 0, None) == -1  # no such form
