"""The ctx = NULL route of the witness-only evaluation through the C ABI (bzk_r1cs_mats_load / _from_r1cs / _info / bzk_r1cs_eval on host threads): the
same per-row functions the kernel runs.  Random matrices against the oracle's r1cs_eval; the three MPN circuits at (3, 3, 1), loaded from a
record_matrices synthesis, against the evaluations the generator itself produced (views 1 - 3) and, with one aux value raised by 1, against the first
unsatisfied row that Python integers find; every refusal of the loader and of the call, with the text bzk_last_error(NULL) leaves."""
import ctypes as C
import struct

import numpy as np
import pytest

import r1cs_eval_cases as cases
from bazuka_amd import lib as L
from oracle import pyref as pr
from util import fr_bytes, r1cs_to_csr, synth_r1cs

F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
ZIESHA = F(1)
R = pr.R_MOD


def _csr_abc(r1):
    return [cases.csr_bytes([row[which] for row in r1["rows"]]) for which in range(3)]


@pytest.mark.parametrize("n_mul,fan", [(5, 3), (100, 3), (2000, 3), (40, 700)])
def test_random_matrices_match_the_oracle(co, n_mul, fan):
    r1 = synth_r1cs(n_mul, fan=fan)
    A, B, Cm = r1cs_to_csr(co, r1)
    zb = fr_bytes(r1["z"])
    mh = L.r1cs_mats_load(_csr_abc(r1), r1["n_in"], r1["n_aux"])
    try:
        info = L.r1cs_mats_info(mh)
        assert (info["n_rows"], info["n_vars"]) == (len(r1["rows"]), len(r1["z"]))
        assert [info["nnzA"], info["nnzB"], info["nnzC"]] == [sum(len(row[k]) for row in r1["rows"]) for k in range(3)]
        assert info["n_coeffs"] == len({c for row in r1["rows"] for k in range(3) for _, c in row[k]})
        az, bz, cz, first = L.r1cs_eval(mh, zb, want_unsat=True)
        assert (az, bz, cz) == co.r1cs_eval(A, B, Cm, zb) and first == -1
        assert L.r1cs_eval(mh, zb) == (az, bz, cz)
    finally:
        L.r1cs_mats_free(mh)


def _world(n_acc):
    w = L.MpnWorld(3, 3)
    for i in range(n_acc):
        w.add_account(i, b"acct%d" % i, ZIESHA, 10 ** 12)
    return w


def _update():
    w = _world(4)
    w.push_tx(0, 1, ZIESHA, 1000, ZIESHA, 7)
    w.push_tx(1, 2, ZIESHA, 500, ZIESHA, 3)
    w.push_tx(0, 3, ZIESHA, 999, ZIESHA, 11)
    return w.update_synthesize(1, F(456), ZIESHA, record_matrices=True)


def _deposit():
    w = _world(2)
    w.add_key(5, b"fresh")
    w.push_deposit(0, ZIESHA, 1000)
    w.push_deposit(5, ZIESHA, 77)
    return w.deposit_synthesize(1, F(456), record_matrices=True)


def _withdraw():
    w = _world(3)
    w.push_withdraw(0, ZIESHA, 500, ZIESHA, 3, F(1234))
    w.push_withdraw(1, ZIESHA, 1, ZIESHA, 0, F(99))
    return w.withdraw_synthesize(1, F(8), record_matrices=True)


def _first_unsat_by_python(r, z, v):
    """the first row that reads variable v and does not hold under the witness z (bytes): every other row holds as it did"""
    mats, touched = [], set()
    for x in "ABC":
        rp = np.frombuffer(r.view("rp" + x), dtype=np.uint32).astype(np.int64)
        col = np.frombuffer(r.view("col" + x), dtype=np.uint32)
        mats.append((rp, col, r.view("val" + x)))
        hits = np.nonzero(col == v)[0]
        touched |= set((np.searchsorted(rp, hits, side="right") - 1).tolist())
    assert touched

    def dot(m, i):
        rp, col, val = m
        return sum(U(val[32 * e:32 * e + 32]) * U(z[32 * int(col[e]):32 * int(col[e]) + 32]) for e in range(int(rp[i]), int(rp[i + 1]))) % R

    for i in sorted(touched):
        if dot(mats[0], i) * dot(mats[1], i) % R != dot(mats[2], i):
            return i
    return -1


@pytest.mark.parametrize("make", [_update, _deposit, _withdraw], ids=["update", "deposit", "withdraw"])
def test_mpn_circuits_from_a_recorded_instance(make):
    r = make()
    assert r.satisfied and r.accepted >= 2
    mh = L.r1cs_mats_from(r)
    try:
        info = L.r1cs_mats_info(mh)
        assert (info["n_rows"], info["n_vars"], info["nnzA"], info["nnzB"], info["nnzC"]) == (r.n_constraints, r.n_in + r.n_aux, r.nnzA, r.nnzB, r.nnzC)
        z = r.view("z")
        az, bz, cz, first = L.r1cs_eval(mh, z, want_unsat=True)
        assert az == r.view("az") and bz == r.view("bz") and cz == r.view("cz")
        assert first == -1
        # one aux value that some row of A reads, raised by 1
        col = np.frombuffer(r.view("colA"), dtype=np.uint32)
        v = int(next(c for c in col[len(col) // 2:] if c >= r.n_in))
        bad = bytearray(z)
        bad[32 * v:32 * v + 32] = F((U(z[32 * v:32 * v + 32]) + 1) % R)
        want = _first_unsat_by_python(r, bytes(bad), v)
        assert want >= 0
        assert L.r1cs_eval(mh, bytes(bad), want_unsat=True)[3] == want
    finally:
        L.r1cs_mats_free(mh)


def test_an_instance_without_matrices_is_refused():
    w = _world(2)
    w.push_deposit(0, ZIESHA, 1)
    r = w.deposit_synthesize(1, F(456))
    with pytest.raises(L.BzkError, match="record_matrices") as e:
        L.r1cs_mats_from(r)
    assert e.value.status == -1


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def _u32(*xs):
    return struct.pack(f"<{len(xs)}I", *xs)


GOOD = (3, _u32(0, 2, 2, 3), _u32(0, 3, 1), F(1) + F(R - 1) + F(5))  # 3 rows over 4 variables


def _with(**kw):
    n_rows, rp, col, val = GOOD
    return (kw.get("n_rows", n_rows), kw.get("rp", rp), kw.get("col", col), kw.get("val", val))


LOAD_REFUSALS = [
    ("n_rows differ", (GOOD, _with(n_rows=2, rp=_u32(0, 2, 3)), GOOD), 2, 2, ("matrix B", "2 rows")),
    ("row_ptr[0] != 0", (_with(rp=_u32(1, 2, 2, 3)), GOOD, GOOD), 2, 2, ("matrix A", "row 0")),
    ("row_ptr descends", (GOOD, GOOD, _with(rp=_u32(0, 2, 1, 3))), 2, 2, ("matrix C", "row 1")),
    ("column out of range", (GOOD, _with(col=_u32(0, 3, 4)), GOOD), 2, 2, ("matrix B", "row 2", "column 4")),
    ("column out of range for the shape", (GOOD, GOOD, GOOD), 2, 1, ("matrix A", "row 0", "column 3")),
    ("coefficient = r", (GOOD, GOOD, _with(val=F(1) + R.to_bytes(32, "little") + F(5))), 2, 2, ("matrix C", "row 0", ">= r")),
    ("coefficient = 2^256 - 1", (_with(val=F(1) + F(2) + b"\xff" * 32), GOOD, GOOD), 2, 2, ("matrix A", "row 2", ">= r")),
    ("col NULL with entries", (_with(col=None), GOOD, GOOD), 2, 2, ("matrix A", "col is NULL")),
    ("val NULL with entries", (GOOD, _with(val=None), GOOD), 2, 2, ("matrix B", "val is NULL")),
    ("row_ptr NULL", (GOOD, GOOD, _with(rp=None)), 2, 2, ("matrix C", "row_ptr is NULL")),
    ("n_in = 0", (GOOD, GOOD, GOOD), 0, 4, ("n_in = 0",)),
]


@pytest.mark.parametrize("name,abc,n_in,n_aux,must", LOAD_REFUSALS, ids=[c[0] for c in LOAD_REFUSALS])
def test_load_refusals_name_the_matrix_and_the_row(name, abc, n_in, n_aux, must):
    with pytest.raises(L.BzkError) as e:
        L.r1cs_mats_load(abc, n_in, n_aux)
    assert e.value.status == -1
    for text in must:
        assert text in str(e.value), (name, str(e.value))


def test_the_good_triple_loads_and_empty_matrices_do():
    mh = L.r1cs_mats_load((GOOD, GOOD, GOOD), 2, 2)
    z = [1, 7, 11, R - 2]
    az, bz, cz = L.r1cs_eval(mh, fr_bytes(z))
    assert az == bz == cz == fr_bytes([(1 - (R - 2)) % R, 0, 35])
    L.r1cs_mats_free(mh)
    empty = (2, _u32(0, 0, 0), None, None)  # NULL col / val with no entries
    mh = L.r1cs_mats_load((empty, empty, empty), 1, 0)
    assert L.r1cs_eval(mh, fr_bytes([1]), want_unsat=True) == (bytes(64), bytes(64), bytes(64), -1)
    L.r1cs_mats_free(mh)


def test_call_refusals_on_the_host_route():
    lib = L.load_library()
    mh = L.r1cs_mats_load((GOOD, GOOD, GOOD), 2, 2)
    z = fr_bytes([1, 7, 11, 13])
    for bad_z in (z[:-32], z + bytes(32)):
        with pytest.raises(L.BzkError, match="variables") as e:
            L.r1cs_eval(mh, bad_z)
        assert e.value.status == -1
    out = C.create_string_buffer(96)
    assert lib.bzk_r1cs_eval(None, mh, None, 4, out, None, None, None) == -1 and b"z is NULL" in lib.bzk_last_error(None)
    assert lib.bzk_r1cs_eval(None, None, z, 4, out, None, None, None) == -1
    assert lib.bzk_r1cs_eval_dev(None, mh, z, 4, out, None, None, 4) == -1  # the device form needs a context
    assert out.raw == bytes(96)                                               # nothing was written
    assert lib.bzk_r1cs_mats_info(None, (C.c_uint64 * 8)()) == -1
    assert L.r1cs_eval(mh, z)[0] == fr_bytes([(1 - 13) % R, 0, 35])          # the handle still evaluates
    L.r1cs_mats_free(mh)
    lib.bzk_r1cs_mats_free(None, None)                                        # a no-op
