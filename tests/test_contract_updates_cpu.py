"""bzk_contract_updates_check with ctx = NULL (the per-lane functions on host threads) and bzk_l1_tx_updates, against the restatements of
tests/contract_update_cases.py: the positive chain and what moving its height, state or counts must clear; the payment-count table; one fault per
row; the refusals (BZK_E_ARG, nothing written); the span helper on the UpdateContract records of tests/l1_tx_cases.py; and the parser under the
address / undefined-behaviour sanitizers as a stand-alone child process."""
import ctypes as C
import functools
import os
import struct
import subprocess

import pytest

import bincode_ref as B
import contract_update_cases as K
import l1_tx_cases as X
from bazuka_amd import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG = -1


def _blob(updates):
    return b"".join(K.enc(u) for u in updates)


def _host(updates, counts, height0=K.HEIGHT0, state0=K.STATE0, desc=None):
    return L.host_contract_updates_check(desc or K.desc(L), _blob(updates), counts, height0, state0)


def _raw(desc, blob, counts, fill=0xA5, capacity_desc=None):
    """the C call on buffers filled with a pattern: (status, ok, aux, commit buffers as bytes)"""
    lib = L.load_library()
    n = sum(counts)
    cnt = (C.c_uint64 * max(len(counts), 1))(*counts)
    bufs = [C.create_string_buffer(bytes([fill]) * k, k) for k in (n + 8, 32 * n + 8, 32 * n + 8)]
    st = lib.bzk_contract_updates_check(None, C.byref(desc.c), L._ptr(blob) if blob else None, len(blob), cnt, len(counts), K.HEIGHT0,
                                        L._ptr(K.STATE0), *bufs)
    return st, [b.raw for b in bufs]


@functools.lru_cache(maxsize=None)
def chain_result():
    ups, counts = K.chain()
    return _host(list(ups), counts)


def test_positive_chain_matches_the_oracles():
    ups, counts = K.chain()
    ok, aux, commit = chain_result()
    want_ok, want_aux, want_commit = K.expected(list(ups), counts, K.HEIGHT0, K.STATE0)
    assert want_ok == bytes([7] * 6)  # the oracle's own verifier accepts every proof of the chain
    assert ok == want_ok
    assert aux == want_aux
    assert commit == want_commit
    kinds = [u["data"][0] for u in ups]
    assert sorted(set(zip(kinds, (u["circuit_id"] for u in ups)))) == sorted((k, i) for k in ("Deposit", "Withdraw", "FunctionCall") for i in (0, 1))


@pytest.mark.parametrize("what, kwargs, cleared", [
    ("height0 + 1: every update is checked at another height", {"height0": K.HEIGHT0 + 1}, {0, 1, 2, 3, 4, 5}),
    ("a wrong state0 breaks the first update only: the others follow their predecessor's claim", {"state0": X.scalar("not the state")}, {0}),
    ("count (2, 2, 2): the fifth update moves to the last transaction's height", {"counts": (2, 2, 2)}, {4}),
    ("count (2, 4, 0): the sixth update moves to the middle transaction's height", {"counts": (2, 4, 0)}, {5}),
    ("count (3, 2, 1): the third update moves to the first transaction's height", {"counts": (3, 2, 1)}, {2}),
])
def test_chain_semantics(what, kwargs, cleared):
    ups, counts = K.chain()
    ok, aux, commit = _host(list(ups), kwargs.pop("counts", counts), **kwargs)
    assert ok == bytes(7 - K.PROOF if i in cleared else 7 for i in range(6)), what
    assert (aux, commit) == chain_result()[1:]  # neither depends on height, state or counts


@functools.lru_cache(maxsize=None)
def count_expected():
    return tuple(K.expected([u], (1,), K.HEIGHT0, K.STATE0) for _, u in K.count_rows())


def test_payment_counts():
    over = 0
    for (label, u), want in zip(K.count_rows(), count_expected()):
        got = _host([u], (1,))
        assert got == want, label
        over += not (want[0][0] & K.ROUTE)
        assert want[0][0] in (7, K.SIGS), (label, want[0][0])  # within capacity: everything holds; beyond: ROUTE and with it PROOF are clear
    assert over == 2  # 5 at capacity 1 and 65 at capacity 3
    # an empty update's aux is the default of its capacity, capacity 0 with one payment the single leaf: both differ from every other row's
    assert len({w[1] for w in count_expected()}) == len(count_expected()) - over + 1


@functools.lru_cache(maxsize=None)
def fault_expected():
    return tuple(K.expected([u], (1,), K.HEIGHT0, K.STATE0) for _, u, _ in K.fault_rows())


def test_one_fault_rows():
    for (label, u, bit), want in zip(K.fault_rows(), fault_expected()):
        got = _host([u], (1,))
        assert got == want, label
        ok = got[0][0]
        if bit == K.UNSUPPORTED:
            assert ok == K.UNSUPPORTED, label
        elif bit == K.ROUTE:
            assert ok == K.SIGS and got[1] == bytes(32), label  # without ROUTE the proof is not looked at and aux is zeros
        else:
            assert ok == 7 - bit, label


def test_key_the_single_verifier_refuses():
    """a function whose key has n_ic != 6 verifies nothing; the other groups of the call are not touched by it"""
    ups, counts = K.chain()
    d, w, f = K.tables()
    short = f[0][:870] + (5).to_bytes(8, "little") + f[0][878:878 + 5 * 97]
    ok, aux, commit = _host(list(ups), counts, desc=K.desc(L, fns=[short, f[1]]))
    assert ok == bytes(7 - K.PROOF if (u["data"][0], u["circuit_id"]) == ("FunctionCall", 0) else 7 for u in ups)
    assert (aux, commit) == chain_result()[1:]


def test_empty_call_is_a_noop():
    st, bufs = _raw(K.desc(L), b"", ())
    assert st == 0 and all(set(b) == {0xA5} for b in bufs)
    assert L.host_contract_updates_check(K.desc(L), b"", (0, 0), 5, K.STATE0) == (b"", b"", b"")


def test_recorded_fixture_is_what_the_oracles_say():
    """tests/golden/contract_update_cases.json (read by the GPU tests) against a fresh run of the generators and restatements"""
    assert (K.fixture(), K.fixture_bin()) == K.build_fixture()
    assert K.recorded_tables() == tuple(K.tables())
    # and the records the GPU tests rebuild from the recorded proofs are the oracle-made ones
    assert [K.enc(u) for u in K.chain(True)[0]] == [K.enc(u) for u in K.chain()[0]]
    assert [K.enc(u) for _, u in K.count_rows(True)] == [K.enc(u) for _, u in K.count_rows()]
    assert [K.enc(u) for _, u, _ in K.fault_rows(True)] == [K.enc(u) for _, u, _ in K.fault_rows()]
    assert K.enc(K.repeatable_call(True)) == K.enc(K.repeatable_call())
    assert all(K.enc(K.crossing_update(i, True)[0]) == K.enc(K.crossing_update(i)[0]) for i in range(8))


# ---- refusals
def _boundaries(u):
    """every field boundary of bincode(u): the record's own fields and, for a payment list, the fields of its first payment"""
    at, out = 0, []
    for name in K.FIELD_ORDER:
        t = dict(zip(K.FIELD_ORDER, (B.U32, K.ContractUpdateData, B.ZkCompressedState, B.L1PublicKey, B.U64, B.ZkProof)))[name]
        if name == "data":
            kind, payload = u["data"]
            out.append(at + 4)  # after the enum tag
            if kind in ("Deposit", "Withdraw"):
                pays = payload["deposits" if kind == "Deposit" else "withdraws"]
                out.append(at + 12)  # after the list's length
                p = at + 12
                schema = [("memo", B.STRING), ("contract_id", B.ContractId), ("circuit", B.U32), ("calldata", B.ZkScalar), ("key", B.L1PublicKey),
                          ("amount", B.Money), ("fee", B.Money)] + ([("nonce", B.U32), ("sig", B.Option(B.L1Signature))] if kind == "Deposit" else [])
                names = {"circuit": "deposit_circuit_id" if kind == "Deposit" else "withdraw_circuit_id", "key": "src" if kind == "Deposit" else "dst"}
                for fname, ft in schema:
                    p += len(ft.enc(pays[0][names.get(fname, fname)]))
                    out.append(p)
                out.append(p - 64 if kind == "Deposit" else p)  # after the Option tag
        at += len(t.enc(u[name]))
        out.append(at)
    return sorted(set(b for b in out if b < at))


def _refusal_cases():
    ups, _ = K.chain()
    return [ups[0], ups[2], ups[1], K.fault_rows()[-1][1]]  # a Deposit, a Withdraw, a FunctionCall, a Mint


def test_refusals_write_nothing():
    desc = K.desc(L)
    lib = L.load_library()
    tried = 0
    for u in _refusal_cases():
        rec = K.enc(u)
        assert _raw(desc, rec, (1,))[0] == 0
        cuts = _boundaries(u)
        assert len(cuts) >= 6
        for cut in [0] + cuts:
            st, bufs = _raw(desc, rec[:cut], (1,))
            assert st == E_ARG and all(set(b) == {0xA5} for b in bufs), (u["data"][0], cut)
            assert (b"record 0" if cut else b"counts") in lib.bzk_mpn_work_last_error()
            tried += 1
        st, bufs = _raw(desc, rec + b"\0", (1,))  # trailing bytes
        assert st == E_ARG and all(set(b) == {0xA5} for b in bufs)
        st, bufs = _raw(desc, rec[:4] + struct.pack("<I", 4) + rec[8:], (1,))  # ContractUpdateData has four variants
        assert st == E_ARG and all(set(b) == {0xA5} for b in bufs)
        proof_tag = len(rec) - 391
        st, bufs = _raw(desc, rec[:proof_tag] + struct.pack("<I", 1) + rec[proof_tag + 4:], (1,))  # ZkProof has one
        assert st == E_ARG and all(set(b) == {0xA5} for b in bufs)
    assert tried > 40
    dep = K.enc(_refusal_cases()[0])
    at = 16  # the first payment's ContractId tag: after circuit_id, the enum tag, the list's length and the memo
    at = 16 + len(B.STRING.enc(_refusal_cases()[0]["data"][1]["deposits"][0]["memo"]))
    st, bufs = _raw(desc, dep[:at] + struct.pack("<I", 3) + dep[at + 4:], (1,))  # ContractId has three variants
    assert st == E_ARG and all(set(b) == {0xA5} for b in bufs)
    # two records where the count says three, and the other way round
    two = dep + K.enc(_refusal_cases()[2])
    assert _raw(desc, two, (1, 1))[0] == 0
    for counts in ((1, 2), (1,)):
        st, bufs = _raw(desc, two, counts)
        assert st == E_ARG and all(set(b) == {0xA5} for b in bufs), counts


def test_record_longer_than_2p20_bytes_is_refused():
    """the documented limit (max_block_size): the longest record that fits is taken - its 7 000-odd withdrawals exceed every capacity, so ROUTE
    is clear - and one withdrawal more is refused with nothing written"""
    desc, lib = K.desc(L), L.load_library()
    per = len(K.long_withdraw_record(2, 0)) - len(K.long_withdraw_record(1, 0))
    k = ((1 << 20) - len(K.long_withdraw_record(0, 0))) // per
    fits, over = K.long_withdraw_record(k, 0), K.long_withdraw_record(k + 1, 0)
    assert len(fits) <= 1 << 20 < len(over) and k > 7000
    assert fits[:5000] == K.enc(K.long_withdraw_update(k, 0))[:5000] and len(fits) == len(K.enc(K.long_withdraw_update(k, 0)))
    st, bufs = _raw(desc, fits, (1,))
    assert st == 0 and bufs[0][0] == K.SIGS and bufs[1][:32] == bytes(32)
    st, bufs = _raw(desc, over, (1,))
    assert st == E_ARG and all(set(b) == {0xA5} for b in bufs)
    assert b"record 0" in lib.bzk_mpn_work_last_error() and b"longer than 1048576" in lib.bzk_mpn_work_last_error()
    st, bufs = _raw(desc, K.enc(_refusal_cases()[2]) + over, (1, 1))   # and as a later record of a call
    assert st == E_ARG and all(set(b) == {0xA5} for b in bufs) and b"record 1" in lib.bzk_mpn_work_last_error()


def test_argument_refusals_name_their_reason():
    lib = L.load_library()
    desc, rec = K.desc(L), K.enc(_refusal_cases()[2])
    ok = C.create_string_buffer(8)
    assert lib.bzk_contract_updates_check(None, C.byref(desc.c), L._ptr(rec), len(rec), None, 1, 0, L._ptr(K.STATE0), ok, None, None) == E_ARG
    assert b"count is NULL" in lib.bzk_mpn_work_last_error()
    broken = K.desc(L)
    broken.c.withdraw_fns = None
    cnt = (C.c_uint64 * 1)(1)
    assert lib.bzk_contract_updates_check(None, C.byref(broken.c), L._ptr(rec), len(rec), cnt, 1, 0, L._ptr(K.STATE0), ok, None, None) == E_ARG
    assert b"function table is NULL" in lib.bzk_mpn_work_last_error()


def test_capacity_nine_is_refused():
    d, w, f = K.tables()
    rec = K.enc(_refusal_cases()[2])
    for desc in (K.desc(L, deposit_fns=[(d[0][0], 9)]), K.desc(L, withdraw_fns=[w[0], (w[1][0], 9)])):
        st, bufs = _raw(desc, rec, (1,))
        assert st == E_ARG and all(set(b) == {0xA5} for b in bufs)
    assert _raw(K.desc(L, deposit_fns=[(d[0][0], 8)]), rec, (1,))[0] == 0
    assert _raw(K.desc(L, fns=[]), rec, (1,))[1][0][0] == K.SIGS  # no such function: ROUTE, not a refusal


def test_null_pointers_with_records_are_refused():
    lib = L.load_library()
    desc, rec = K.desc(L), K.enc(_refusal_cases()[2])
    cnt = (C.c_uint64 * 1)(1)
    ok = C.create_string_buffer(8)
    good = [None, C.byref(desc.c), L._ptr(rec), len(rec), cnt, 1, 0, L._ptr(K.STATE0), ok, None, None]
    assert lib.bzk_contract_updates_check(*good) == 0
    for at in (1, 2, 4, 7, 8):
        args = list(good)
        args[at] = None
        assert lib.bzk_contract_updates_check(*args) == E_ARG, at


# ---- bzk_l1_tx_updates
def test_l1_tx_updates_spans():
    cid = X.scalar("cid")
    nothing = L.ContractDesc(cid)  # no functions: every update is well-formed and routed nowhere
    for form in (X.FORM_TX, X.FORM_TX_AND_DELTA):
        records = [rec for label, rec in X.corpus(form) if label.startswith(("variant", "UpdateContract"))]
        txs = b"".join(records)
        n_found, spans = L.l1_tx_updates(txs, len(records), cid, form)
        assert n_found == len(spans) and n_found % 4 == 0 and n_found >= 8  # the variant's four updates in every UpdateContract record that has them
        starts = [sum(len(r) for r in records[:i]) for i in range(len(records) + 1)]
        for k in range(0, n_found, 4):
            group = spans[k:k + 4]
            tx = group[0][0]
            assert all(t == tx and starts[tx] <= off and off + length <= starts[tx + 1] for t, off, length in group)
            blob = b"".join(txs[off:off + length] for _, off, length in group)
            values = [B.decode(K.ContractUpdate, txs[off:off + length]) for _, off, length in group]  # each span is one whole record
            assert [v["data"][0] for v in values] == ["Deposit", "Withdraw", "FunctionCall", "Mint"]
            ok, aux, commit = L.host_contract_updates_check(nothing, blob, (4,), 0, bytes(32))  # accepted as well-formed
            assert ok == bytes([0, K.SIGS, K.SIGS, K.UNSUPPORTED])  # no function to route to; the deposit's signature is any 64 bytes
            assert commit == b"".join(K.F(K.commit_of(v["prover"], v["reward"])) for v in values)
        assert L.l1_tx_updates(txs, len(records), X.scalar("another contract"), form) == (0, [])
        assert L.l1_tx_updates(txs, len(records), cid, form, cap=3) == (n_found, spans[:3])
        assert L.l1_tx_updates(txs, len(records), cid, form, cap=0) == (n_found, [])
    with pytest.raises(L.BzkError):
        L.l1_tx_updates(txs[:-1], len(records), cid, X.FORM_TX_AND_DELTA)


# ---- the parser under the sanitizers
def test_parser_under_sanitizers(tmp_path):
    exe = os.path.join(HERE, "host", "_updates_parse_check")
    if not os.path.exists(exe):
        pytest.skip("tests/host/_updates_parse_check not built (build() compiles it)")
    ups, _ = K.chain()
    cases = [K.enc(u) for u in (ups[0], ups[2], ups[1], K.fault_rows()[-1][1], K.fault_rows()[1][1])]
    path = tmp_path / "records.bin"
    path.write_bytes(K.CID_BYTES + struct.pack("<I", len(cases)) + b"".join(struct.pack("<I", len(c)) + c for c in cases))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "5 records" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
