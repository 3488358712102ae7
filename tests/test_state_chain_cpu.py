"""bzk_state_update_chain without a GPU: the surface of the three new entry points, their argument checks, bzk_l1_tx_deltas against records built
with tests/l1_tx_cases.py, and the chain planner (bazuka_amd/csrc/bzk_state_chain.h) driven by tests/host/state_chain_check.hip against a value
store in host memory - every group hashed with poseidon29_hash<T> on the host - over cases written here with tests/pystate.py: the model, the
deltas, and the (hash, size) PyKvState gives after every delta."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import pytest

import bincode_ref as B
import l1_tx_cases as X
import pystate as ps
from bazuka_amd import lib as L
from oracle import pyref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("bzk_state_update_chain", "bzk_state_update_chain_bincode", "bzk_l1_tx_deltas")
S = ("scalar",)
F = pr.fr_to_mont_bytes
E_ARG = -1


# ---- surface: header = exports = ctypes = bzk-sys
def test_new_names_on_every_surface():
    header = open(os.path.join(ROOT, "include", "bzk.h")).read()
    sys_rs = open(os.path.join(ROOT, "rust", "bzk-sys", "src", "lib.rs")).read()
    lib = L.load_library()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in L.SIGNATURES and getattr(lib, name) is not None, name
        assert re.search(r"pub fn %s\(" % name, sys_rs), name
    for k, v in (("APPLIED", 0), ("MISMATCH", 1), ("REFUSED", 2), ("NOT_REACHED", 3)):
        assert re.search(r"#define BZK_CHAIN_%s\s+%du" % (k, v), header) and getattr(L, "CHAIN_" + k) == v


def test_chain_entries_refuse_null_arguments_without_a_device():
    lib = L.load_library()
    one = (C.c_uint64 * 2)(0, 0)
    out, verdict, applied = C.create_string_buffer(40), C.create_string_buffer(1), C.c_uint64(7)
    # a NULL handle, whatever else is given
    assert lib.bzk_state_update_chain(None, 1, one, one, one, None, one, None, 0, out, verdict, C.byref(applied), None) == E_ARG
    assert lib.bzk_state_update_chain_bincode(None, 1, b"\0" * 8, one, one, None, 0, out, verdict, C.byref(applied)) == E_ARG
    assert lib.bzk_state_update_chain(None, 0, None, None, None, None, None, None, 0, None, None, None, None) == E_ARG
    assert applied.value == 7 and out.raw == bytes(40)
    # NULL arrays with m > 0: refused before the handle is looked at (the bytes behind this pointer are no state)
    fake = C.create_string_buffer(4096)
    for args in ((None, one, one, None, one, None, 0, out, verdict, C.byref(applied), None),
                 (one, one, one, None, None, None, 0, out, verdict, C.byref(applied), None),
                 (one, one, one, None, one, None, 0, None, verdict, C.byref(applied), None),
                 (one, one, one, None, one, None, 0, out, None, C.byref(applied), None),
                 (one, one, one, None, one, None, 0, out, verdict, None, None)):
        assert lib.bzk_state_update_chain(fake, 1, *args) == E_ARG
    for args in ((None, one, one, None, 0, out, verdict, C.byref(applied)), (b"\0" * 8, None, one, None, 0, out, verdict, C.byref(applied)),
                 (b"\0" * 8, one, None, None, 0, out, verdict, C.byref(applied)), (b"\0" * 8, one, one, None, 0, None, verdict, C.byref(applied)),
                 (b"\0" * 8, one, one, None, 0, out, None, C.byref(applied)), (b"\0" * 8, one, one, None, 0, out, verdict, None)):
        assert lib.bzk_state_update_chain_bincode(fake, 1, *args) == E_ARG
    down = (C.c_uint64 * 2)(8, 0)  # byte offsets that do not ascend
    assert lib.bzk_state_update_chain_bincode(fake, 1, b"\0" * 8, down, one, None, 0, out, verdict, C.byref(applied)) == E_ARG
    assert applied.value == 7


# ---- bzk_l1_tx_deltas
def _update_tx(cid_tag, delta, memo):
    data = ("UpdateContract", {"contract_id": ("Custom", X.scalar(cid_tag)), "updates": [X.contract_update("FunctionCall", {"fee": X.money(4)}, memo)],
                               "delta": delta})
    return X.sign_tx(b"wallet " + memo.encode(), X.tx_of(data, memo=memo))


def test_l1_tx_deltas_spans():
    cid = X.scalar("cid")
    inside, outside = X.delta_pairs(3), X.delta_pairs(5)
    body_in, body_out = B.encode(X.ZkDeltaPairs, inside), B.encode(X.ZkDeltaPairs, outside)
    # (transaction, its trailing state_delta, expected source): a delta inside, one in state_delta, both, neither, another contract's, no UpdateContract
    rows = [(_update_tx("cid", inside, "in"), None, 0), (_update_tx("cid", None, "sd"), outside, 1), (_update_tx("cid", inside, "both"), outside, 0),
            (_update_tx("cid", None, "none"), None, 2), (_update_tx("another", inside, "other"), outside, None), (X.variant_txs()[4], outside, None)]
    records = [X.enc(tx, X.FORM_TX_AND_DELTA, state_delta=sd) for tx, sd, _ in rows]
    txs = b"".join(records)
    starts = [sum(len(r) for r in records[:i]) for i in range(len(records) + 1)]
    found, spans = L.l1_tx_deltas(txs, len(records), cid, X.FORM_TX_AND_DELTA)
    want_src = [(i, src) for i, (_, _, src) in enumerate(rows) if src is not None]
    assert found == len(spans) == len(want_src) == 4
    for (tx, off, length, src), (i, want) in zip(spans, want_src):
        assert (tx, src) == (i, want)
        if src == 2:
            assert length == 0
            continue
        assert starts[tx] <= off and off + length <= starts[tx + 1]
        assert txs[off:off + length] == (body_in if src == 0 else body_out)
        assert txs[off - 1] == 1  # the Option's tag in front of the body
    assert L.l1_tx_deltas(txs, len(records), cid, X.FORM_TX_AND_DELTA, cap=2) == (4, spans[:2])
    assert L.l1_tx_deltas(txs, len(records), cid, X.FORM_TX_AND_DELTA, cap=0) == (4, [])
    assert L.l1_tx_deltas(txs, len(records), X.scalar("another"), X.FORM_TX_AND_DELTA)[1] == [(4, spans[0][1] - starts[0] + starts[4], len(body_in), 0)]
    # plain Transaction records: only the delta inside counts
    plain = [X.enc(tx, X.FORM_TX) for tx, _, _ in rows]
    found, spans = L.l1_tx_deltas(b"".join(plain), len(plain), cid, X.FORM_TX)
    assert [(t, s) for t, _, _, s in spans] == [(0, 0), (1, 2), (2, 0), (3, 2)]
    # a truncated input: refused, n_out = 0, nothing written
    lib = L.load_library()
    n_out, buf = C.c_uint64(9), (C.c_uint64 * 16)(*([5] * 16))
    assert lib.bzk_l1_tx_deltas(txs[:-1], len(txs) - 1, len(records), X.FORM_TX_AND_DELTA, cid, buf, 4, C.byref(n_out)) == E_ARG
    assert n_out.value == 0 and list(buf) == [5] * 16
    with pytest.raises(L.BzkError):
        L.l1_tx_deltas(txs[:-1], len(records), cid, X.FORM_TX_AND_DELTA)


# ---- the planner under the sanitizers
def _case(model, deltas, refused_at=None):
    """deltas: lists of (locator, value) - value an int, None, or 32 raw bytes (a refused delta may hold anything)"""
    out = [struct.pack("<Q", len(ps.model_bincode(model))), ps.model_bincode(model), struct.pack("<Q", len(deltas))]
    for d in deltas:
        d = list(d.items()) if isinstance(d, dict) else d
        out.append(struct.pack("<Q", len(d)))
        for loc, v in d:
            out.append(struct.pack("<Q", len(loc)) + b"".join(struct.pack("<Q", x) for x in loc))
            out.append(v if isinstance(v, bytes) else F((v or 0) % pr.R_MOD))
    k = len(deltas) if refused_at is None else refused_at
    ref = ps.PyKvState(model)
    out.append(struct.pack("<Q", k))
    for j, d in enumerate(deltas[:k]):
        ref.update_contract(d if isinstance(d, dict) else dict(d), j)
        out.append(F(ref.hash) + struct.pack("<Q", ref.size))
    return b"".join(out)


def _cases():
    st2, lst = ("struct", [S, S]), ("list", 3, ("struct", [S, S]))
    cases = [
        # the reference's three state scripts (src/zk/test/mod.rs:64-287) as chains
        _case(S, [{(): 0xF}]),
        _case(st2, [{(0,): 0xF}, {(1,): 0xF0}, {(0,): 0xF00}, {(0,): 0xF}, {(0,): 0, (1,): 0}]),
        _case(lst, [{(62, 0): 0xF00000}, {(33, 0): 0xF}, {(33, 1): 0xF0}, {(33, 0): 0xF00}, {(33, 0): 0xF}, {(33, 0): 0, (33, 1): 0}, {(62, 0): 0}]),
        # List{0, ..}: the list and its only item share a slot
        _case(("struct", [S, ("list", 0, ("struct", [S, S])), ("list", 0, S)]), [{(1, 0, 0): 5}, {(2, 0): 6, (0,): 1}, {(1, 0, 1): 7, (2, 0): 0}, {(2, 0): 9}]),
        _case(("list", 0, ("list", 0, S)), [{(0, 0): 5}, {(0, 0): 6}]),
        # a key created by delta 1 is a sibling delta 2 reads; then an inner node created by one delta under another's path
        _case(("list", 2, S), [{(5,): 7}, {(4,): 9}, {(6,): 1, (12,): 2}, {(13,): 3}, {(5,): 0}]),
        # the same scalar written by three deltas in a row
        _case(("list", 2, S), [{(5,): 1}, {(5,): 2}, {(5,): 0}, {(5,): 2}]),
        # an empty delta first, in the middle and last
        _case(st2, [{}, {(1,): 3}, {}, {}, {(0,): 4}, {}]),
        _case(st2, [{}]),
        # a refused delta at positions 0, middle and last: bad index, not a scalar, below a scalar, a duplicate, a value that is no field element
        _case(lst, [[((64, 0), 1)], {(1, 0): 2}], refused_at=0),
        _case(lst, [{(1, 0): 2}, {(2, 1): 3, (1, 1): 4}, [((3, 0), 1), ((3,), 1)], {(1, 0): 9}], refused_at=2),
        _case(lst, [{(1, 0): 2}, {(2, 1): 3}, [((3, 0, 0), 1)]], refused_at=2),
        _case(lst, [{(1, 0): 2}, [((7, 0), 1), ((7, 0), 1)], {(2, 1): 3}], refused_at=1),
        _case(lst, [{(1, 0): 2}, {(9, 1): 2}, [((8, 0), 1), ((8, 1), b"\xff" * 32)]], refused_at=2),
    ]
    # seeded chains over the account model and a mixed one, over a small index range: the deltas keep meeting
    rnd = random.Random(20)
    for model, m in ((ps.mpn_model(2, 1), 9), (("struct", [S, ("list", 2, ("struct", [S, ("list", 1, S), S])), ("list", 1, S)]), 12)):
        deltas = []
        for _ in range(m):
            d = {}
            for _ in range(rnd.choice([1, 2, 6, 15])):
                loc, cur = [], model
                while cur[0] != "scalar":
                    if cur[0] == "struct":
                        loc.append(rnd.randrange(len(cur[1])))
                        cur = cur[1][loc[-1]]
                    else:
                        loc.append(rnd.randrange(min(4 ** cur[1], 6)))
                        cur = cur[2]
                d[tuple(loc)] = rnd.choice([None, 0, 1, rnd.randrange(pr.R_MOD), pr.R_MOD - 1])
            deltas.append(d)
        cases.append(_case(model, deltas))
    return cases


def test_chain_planner_against_the_restatement_under_sanitizers(tmp_path):
    exe = os.path.join(HERE, "host", "_state_chain_check")
    assert os.path.exists(exe), "tests/host/_state_chain_check not built (build() compiles it)"
    cases = _cases()
    path = tmp_path / "chains.bin"
    path.write_bytes(struct.pack("<Q", len(cases)) + b"".join(cases))
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "state_chain_check ok: %d cases" % len(cases) in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
