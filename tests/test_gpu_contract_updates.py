"""bzk_contract_updates_check on the GPU (bazuka_amd/csrc/updates.hip: upd_deposit_sig, upd_deposit_leaf, upd_withdraw_leaf, upd_tree_level,
upd_inputs, the verifier's three kernels per key group, upd_verdict) against the ctx = NULL call - byte for byte - and against the oracles'
answers recorded in tests/golden/contract_update_cases.json: the records are rebuilt by the generators of tests/contract_update_cases.py from
the keys and proofs that file holds (tests/test_contract_updates_cpu.py checks the file, and that the rebuilt records are the oracle-made ones).
Then the wavefront, level and round edges."""
import functools

import pytest

import bincode_ref as B
import contract_update_cases as K
from bazuka_amd import lib as L

pytestmark = pytest.mark.gpu


def fx():
    return K.fixture()


@functools.lru_cache(maxsize=None)
def desc():
    return K.fixture_desc(L)


def H(x):
    return bytes.fromhex(x)


def both(bzk, blob, counts, height0=K.HEIGHT0, state0=K.STATE0):
    """the device call, asserted byte-equal to the host-thread call"""
    dev = bzk.contract_updates_check(desc(), blob, counts, height0, state0)
    host = L.host_contract_updates_check(desc(), blob, counts, height0, state0)
    assert dev[0] == host[0], [(i, d, h) for i, (d, h) in enumerate(zip(dev[0], host[0])) if d != h][:10]
    assert dev[1] == host[1] and dev[2] == host[2]
    return dev


def test_positive_chain(bzk):
    c = fx()["chain"]
    ups, counts = K.chain(True)
    blob = b"".join(K.enc(u) for u in ups)
    ok, aux, commit = both(bzk, blob, counts)
    assert ok == H(c["ok"]) == bytes([7] * 6)
    assert aux == H(c["aux"]) and commit == H(c["commit"])
    # moved by one height every proof fails, under another state only the first
    assert both(bzk, blob, counts, height0=K.HEIGHT0 + 1)[0] == bytes([6] * 6)
    assert both(bzk, blob, counts, state0=bytes(32))[0] == bytes([6] + [7] * 5)
    assert both(bzk, blob, (2, 2, 2))[0] == bytes([7, 7, 7, 7, 6, 7])


def rows():
    """[(recorded expectations, record bytes)] of the payment-count table and the one-fault rows"""
    recs = [K.enc(u) for _, u in K.count_rows(True)] + [K.enc(u) for _, u, _ in K.fault_rows(True)]
    want = fx()["count_rows"] + fx()["fault_rows"]
    assert [w["label"] for w in want] == [label for label, _ in K.count_rows(True)] + [label for label, _, _ in K.fault_rows(True)]
    return list(zip(want, recs))


def test_payment_counts_and_fault_rows_one_call_each(bzk):
    for row, rec in rows():
        ok, aux, commit = both(bzk, rec, (1,))
        assert (ok[0], aux, commit) == (row["ok"], H(row["aux"]), H(row["commit"])), row["label"]


def test_all_rows_in_one_call(bzk):
    """the same records as ONE call of one transaction: every kind and function, trees of every depth and empty ones share the launches.  Aux,
    commitment, SIGS and ROUTE of a row do not depend on its neighbours; PROOF does (each row was proved against state0), so it is compared with
    the host-thread call only"""
    want, recs = zip(*rows())
    ok, aux, commit = both(bzk, b"".join(recs), (len(recs),))
    assert aux == b"".join(H(r["aux"]) for r in want) and commit == b"".join(H(r["commit"]) for r in want)
    assert bytes(o & 0x86 for o in ok) == bytes(r["ok"] & 0x86 for r in want)
    assert ok[0] == want[0]["ok"]  # the first is checked against state0


@pytest.mark.parametrize("n", [65, 130])
def test_function_calls_across_wavefronts(bzk, n):
    """one valid FunctionCall record whose next_state is state0, repeated in one transaction: every copy stays valid"""
    ok, aux, commit = both(bzk, K.enc(K.repeatable_call(True)) * n, (n,))
    assert ok == bytes([7] * n)
    assert aux == H(fx()["repeatable_aux"]) * n and commit == H(fx()["repeatable_commit"]) * n


def test_levels_with_lanes_from_some_updates_only(bzk):
    """an update of 64 deposits (capacity 3) next to updates of 1 and 0 payments of capacities 1 and 3: levels 2 and 3 have lanes from the deep
    trees only, the empty updates none at all"""
    by_label = {w["label"]: (w, rec) for w, rec in rows()}
    pick = [by_label[k] for k in ("Deposit fn 1 x 64", "Deposit fn 0 x 1", "Deposit fn 1 x 0", "Deposit fn 0 x 0", "Deposit fn 1 x 1", "Withdraw fn 1 x 7",
                              "Deposit fn 0 x 4", "Withdraw fn 0 x 1", "Deposit fn 1 x 17")]
    blob = b"".join(rec for _, rec in pick)
    for counts in ((len(pick),), (1, 0, 3, len(pick) - 4)):
        ok, aux, commit = both(bzk, blob, counts)
        assert aux == b"".join(H(w["aux"]) for w, _ in pick)
        assert bytes(o & 6 for o in ok) == bytes([6] * len(pick))


def test_payment_round_crossing(bzk):
    """1 030 deposit updates of 64 payments: 65 920 payments, so the second round starts at update 1 024"""
    cross = [K.crossing_update(i, True)[0] for i in range(8)]
    want = [H(a) for a in fx()["crossing_aux"]]
    recs = [K.enc(u) for u in cross]
    n = 1030
    blob = b"".join(recs[i % 8] for i in range(n))
    ok, aux, commit = both(bzk, blob, (n,))
    assert ok == bytes([6] * n)  # signed and routed; the proofs are garbage
    for i in (0, 1, 511, 700, 1023, 1024, 1025, 1029):
        assert aux[32 * i:32 * i + 32] == want[i % 8], i
    # and against pystate.compress on the pairs deposit.rs builds: the eight sampled updates are rotations 0, 1, 7, 4, 7, 0, 1, 5 of the
    # pool; all eight rotations are computed here
    for i in range(8):
        u = B.decode(K.ContractUpdate, recs[i])
        assert len(u["data"][1]["deposits"]) == 64 and K.F(K.aux_of("Deposit", u["data"][1], 3)) == want[i]
        assert all(aux[32 * j:32 * j + 32] == want[i] for j in range(i, n, 8))


def test_byte_round_crossing(bzk):
    """68 Withdraw updates of 60 withdrawals with 17 000-byte memos, about 1 MB each: 4 080 payments, so the rounds end at 64 MiB of record bytes
    and not at 2^16 payments.  The repeatable FunctionCall follows every one of them (their next_state is state0) and stays valid on either side
    of the boundary, first in its round or not; the second call shifts the records by one"""
    d3 = K.fixture_desc(L, withdraw_caps=(3, 3))
    long_u = K.long_withdraw_update(60, 17000)
    big, call = K.long_withdraw_record(60, 17000), K.enc(K.repeatable_call(True))
    assert big == K.enc(long_u) and 1000000 < len(big) <= 1 << 20
    want_aux = K.F(K.aux_of("Withdraw", long_u["data"][1], 3))
    pair = big + call
    for lead in (b"", call):
        n = 2 * 68 + (1 if lead else 0)
        blob = lead + pair * 68
        assert len(blob) > (64 << 20) + len(pair)
        dev = bzk.contract_updates_check(d3, blob, (n,), K.HEIGHT0, K.STATE0)
        assert dev == L.host_contract_updates_check(d3, blob, (n,), K.HEIGHT0, K.STATE0)
        ok, aux, commit = dev
        calls = [i for i in range(n) if (i % 2 == 1) != bool(lead)]
        assert all(ok[i] == (7 if i in calls else 6) for i in range(n)), list(ok)
        assert all(aux[32 * i:32 * i + 32] == (H(fx()["repeatable_aux"]) if i in calls else want_aux) for i in range(n))


def test_verifier_round_crossing(bzk):
    """2^16 + 65 copies of the repeatable FunctionCall in one transaction, every 97th with a tampered proof: the key group runs two rounds"""
    n = (1 << 16) + 65
    good, bad = K.enc(K.repeatable_call(True)), K.enc(K.tampered(K.repeatable_call(True)))
    assert len(good) == len(bad)
    blob = b"".join(bad if i % 97 == 96 else good for i in range(n))
    ok, aux, commit = bzk.contract_updates_check(desc(), blob, (n,), K.HEIGHT0, K.STATE0)
    want = bytes(6 if i % 97 == 96 else 7 for i in range(n))
    assert ok[-65:] == want[-65:]
    assert ok == want
    assert aux == H(fx()["repeatable_aux"]) * n


def test_refusal_and_back_to_back_calls(bzk):
    """a refused call writes nothing and leaves the context usable; a second call reuses the workspace"""
    lib = L.load_library()
    rec = K.enc(K.repeatable_call(True))
    cnt = (L.C.c_uint64 * 1)(2)
    ok = L.C.create_string_buffer(b"\x55" * 8, 8)
    short, state0 = rec + rec[:-1], K.STATE0
    st = lib.bzk_contract_updates_check(bzk.h, L.C.byref(desc().c), L._ptr(short), len(short), cnt, 1, K.HEIGHT0, L._ptr(state0), ok, None, None)
    assert st == -1 and ok.raw == b"\x55" * 8 and b"record 1" in lib.bzk_mpn_work_last_error()
    assert both(bzk, rec * 2, (2,))[0] == bytes([7, 7])
    assert bzk.contract_updates_check(desc(), b"", (), 0, bytes(32)) == (b"", b"", b"")
