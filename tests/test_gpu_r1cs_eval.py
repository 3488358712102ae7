"""GPU: A.z, B.z, C.z from the witness alone (bzk_r1cs_mats_*, bzk_r1cs_eval*) and bzk_groth16_prove_witness.  The evaluations are byte for byte the
CPU oracle's r1cs_eval (and, on the structured table, Python integers); a proof from z alone is byte for byte bzk_groth16_prove's on the oracle's
evaluations, which is the oracle prover's.  No shape is larger than 2^12 rows except the MPN Update(3,3,1) circuit (126 001 rows)."""
import ctypes as C
import random
import threading

import pytest
import torch

import r1cs_eval_cases as cases
from bazuka_amd import Bzk, lib as L
from bazuka_amd.lib import BZK_E_UNSAT, BzkError
from oracle import pyref as pr
from util import dev_bytes, fr_bytes, fr_list, log2_ceil, r1cs_to_csr, synth_r1cs, to_dev

pytestmark = pytest.mark.gpu
F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
R = pr.R_MOD
TAIL = 96  # bytes behind the padded outputs that must not change


def _csr_abc(r1):
    return [cases.csr_bytes([row[which] for row in r1["rows"]]) for which in range(3)]


def _eval_dev(bzk, mh, zb, n_rows, pad_rows):
    """r1cs_eval_dev into buffers pre-filled with 0xFF; checks the pad and the bytes behind it, returns the three evaluations"""
    dz = to_dev(zb)
    outs = [torch.full((pad_rows * 32 + TAIL,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    bzk.r1cs_eval_dev(mh, dz, len(zb) // 32, outs[0], outs[1], outs[2], pad_rows)
    bzk.sync()
    got = [dev_bytes(o) for o in outs]
    for g in got:
        assert g[32 * n_rows:32 * pad_rows] == bytes(32 * (pad_rows - n_rows)), "the pad reads back as zeros"
        assert g[32 * pad_rows:] == b"\xff" * TAIL, "nothing behind pad_rows * 32 changes"
    return tuple(g[:32 * n_rows] for g in got)


@pytest.mark.parametrize("n_mul,fan", [(5, 3), (100, 3), (2000, 3), (40, 700)])
def test_eval_dev_matches_the_oracle_on_random_matrices(bzk, co, n_mul, fan):
    r1 = synth_r1cs(n_mul, fan=fan)
    A, B, Cm = r1cs_to_csr(co, r1)
    zb = fr_bytes(r1["z"])
    n_rows = len(r1["rows"])
    mh = bzk.r1cs_mats_load(_csr_abc(r1), r1["n_in"], r1["n_aux"])
    try:
        want = co.r1cs_eval(A, B, Cm, zb, nthreads=co.ncpu())
        assert _eval_dev(bzk, mh, zb, n_rows, 1 << log2_ceil(n_rows)) == want
        assert bzk.r1cs_eval(mh, zb, want_unsat=True) == want + (-1,)   # the host-pointer form: upload, the same launch, read-back
        az_only = torch.full((n_rows * 32,), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bzk.r1cs_eval_dev(mh, to_dev(zb), len(r1["z"]), az_only, None, None, n_rows)  # any output may be NULL
        bzk.sync()
        assert dev_bytes(az_only) == want[0]
    finally:
        bzk.r1cs_mats_free(mh)


@pytest.fixture(scope="module")
def table_witness():
    return cases.witness()


@pytest.mark.parametrize("n_rows", [1, 63, 65, 257])
def test_structured_table_as_a_matrix_triple(bzk, co, table_witness, n_rows):
    """the CPU check's table (tests/r1cs_eval_cases.py) as A, B, C: row counts that leave the last workgroup and the last wave partial"""
    z = table_witness
    abc = cases.triple(n_rows)
    zb = fr_bytes(z)
    mh = bzk.r1cs_mats_load([cases.csr_bytes(m) for m in abc], 1, len(z) - 1)
    try:
        got = _eval_dev(bzk, mh, zb, n_rows, 1 << log2_ceil(n_rows))
        for g, rows in zip(got, abc):
            assert g == fr_bytes(cases.expected(rows, z))
        holders = []
        for rows in abc:
            rp, col, val = [0], [], []
            for row in rows:
                col += [v for v, _ in row]
                val += [F(c) for _, c in row]
                rp.append(len(col))
            holders.append(co.CsrHolder(n_rows, rp, col, b"".join(val)))
        assert got == co.r1cs_eval(*holders, zb, nthreads=co.ncpu())
    finally:
        bzk.r1cs_mats_free(mh)


def test_one_5000_term_row_among_300_one_term_rows(bzk, table_witness):
    z = table_witness
    rnd = random.Random(5000)
    long_row = [(rnd.randrange(len(z)), rnd.choice((1, R - 1, R - 2, rnd.randrange(R)))) for _ in range(5000)]
    rows = [[(rnd.randrange(len(z)), rnd.randrange(R))] for _ in range(300)]
    rows.insert(137, long_row)
    abc = [rows, rows[::-1], rows[100:] + rows[:100]]
    mh = bzk.r1cs_mats_load([cases.csr_bytes(m) for m in abc], 1, len(z) - 1)
    try:
        got = _eval_dev(bzk, mh, fr_bytes(z), 301, 512)
        for g, m in zip(got, abc):
            assert g == fr_bytes(cases.expected(m, z))
    finally:
        bzk.r1cs_mats_free(mh)


# ---- proofs ------------------------------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _proof_case(co, n_mul):
    """(r1, oracle CRS, z bytes, oracle evaluations) per circuit size, made once"""
    if n_mul not in _CASES:
        r1 = synth_r1cs(n_mul, seed=7000 + n_mul)
        A, B, Cm = r1cs_to_csr(co, r1)
        params = co.groth16_setup(A, B, Cm, r1["n_in"], r1["n_aux"], log2_ceil(len(r1["rows"])), fr_bytes(fr_list(5, n_mul + 1)), nthreads=co.ncpu())
        zb = fr_bytes(r1["z"])
        _CASES[n_mul] = (r1, params, zb, co.r1cs_eval(A, B, Cm, zb, nthreads=co.ncpu()))
    return _CASES[n_mul]


def _rs(k):
    b = fr_bytes(fr_list(2, 900 + k))
    return b[:32], b[32:]


@pytest.mark.parametrize("n_mul", [5, 100, 2000])
def test_prove_witness_bytes_equal_prove_and_the_oracle(bzk, co, n_mul):
    r1, params, zb, (az, bz, cz) = _proof_case(co, n_mul)
    if n_mul == 5:
        assert len(r1["rows"]) == 8  # exactly 2^log_m rows: no pad
    r, s = _rs(n_mul)
    ph = bzk.params_load(params)
    mh = bzk.r1cs_mats_load(_csr_abc(r1), r1["n_in"], r1["n_aux"])
    try:
        got = bzk.groth16_prove_witness(ph, mh, zb, r, s)
        assert got == bzk.groth16_prove(ph, zb, az, bz, cz, r, s)
        assert got == co.groth16_prove(params, zb, az, bz, cz, r, s, nthreads=co.ncpu())
        assert bzk.groth16_prove_witness(ph, mh, zb, r, s, check=True) == got
    finally:
        bzk.r1cs_mats_free(mh)
        bzk.params_free(ph)


def test_mpn_update_circuit_from_view_0_alone(bzk):
    w = L.MpnWorld(3, 3)
    for i in range(4):
        w.add_account(i, b"acct%d" % i, F(1), 10 ** 9)
    w.push_tx(0, 1, F(1), 1000, F(1), 7)
    w.push_tx(1, 2, F(1), 500, F(1), 3)
    w.push_tx(2, 3, F(1), 10, F(1), 1)
    r = w.update_synthesize(1, F(456), F(1), record_matrices=True)
    assert r.satisfied and r.accepted == 3
    csr = [(r.n_constraints, r.view("rp" + x), r.view("col" + x), r.view("val" + x)) for x in "ABC"]
    ph, _ = bzk.groth16_setup(csr, r.n_in, r.n_aux, fr_bytes(fr_list(5, 31337)))
    mh = bzk.r1cs_mats_from(r)
    try:
        rb, sb = _rs(1)
        want = bzk.groth16_prove_r1cs(ph, r, rb, sb)
        assert bzk.groth16_prove_witness(ph, mh, r.view("z"), rb, sb, check=True) == want
        assert bzk.r1cs_eval(mh, r.raw("z")) == (r.view("az"), r.view("bz"), r.view("cz"))
    finally:
        bzk.r1cs_mats_free(mh)
        bzk.params_free(ph)


def _first_unsat(r1, z):
    for i, (A, B, Cr) in enumerate(r1["rows"]):
        dot = lambda row: sum(c * z[v] for v, c in row) % R
        if dot(A) * dot(B) % R != dot(Cr):
            return i
    return -1


def test_check_sat_reports_the_first_unsatisfied_row_and_leaves_the_proof_alone(bzk, co):
    r1, params, zb, (az, bz, cz) = _proof_case(co, 100)
    r, s = _rs(5)
    ph = bzk.params_load(params)
    mh = bzk.r1cs_mats_load(_csr_abc(r1), r1["n_in"], r1["n_aux"])
    try:
        want = bzk.groth16_prove(ph, zb, az, bz, cz, r, s)
        assert bzk.groth16_prove_witness(ph, mh, zb, r, s, check=True) == want
        z = list(r1["z"])
        v = r1["n_in"] + 40                     # an aux value in the middle of the circuit
        z[v] = (z[v] + 1) % R
        row = _first_unsat(r1, z)
        assert row >= 0
        out = C.create_string_buffer(b"\xaa" * 387, 387)
        with pytest.raises(BzkError, match=f"constraint {row} is not satisfied") as e:
            bzk.groth16_prove_witness(ph, mh, fr_bytes(z), r, s, check=True, out=out)
        assert e.value.status == BZK_E_UNSAT
        assert out.raw == b"\xaa" * 387         # proof_out untouched
        assert bzk.r1cs_eval(mh, fr_bytes(z), want_unsat=True)[3] == row
        bad = bzk.groth16_prove_witness(ph, mh, fr_bytes(z), r, s)   # without the flag: an (invalid) proof, as bzk_groth16_prove gives
        a2, b2, c2 = co.r1cs_eval(*r1cs_to_csr(co, r1), fr_bytes(z))
        assert bad == bzk.groth16_prove(ph, fr_bytes(z), a2, b2, c2, r, s) and bad != want
        assert bzk.groth16_prove_witness(ph, mh, zb, r, s, check=True) == want   # the next clean proof on the same slot
    finally:
        bzk.r1cs_mats_free(mh)
        bzk.params_free(ph)


def _rewitness(r1, seed):
    """another witness of the same matrices: fresh inputs, every aux value recomputed row by row"""
    rnd = random.Random(seed)
    z = [1] + [rnd.randrange(R) for _ in range(r1["n_in"] - 1)]
    for A, B, Cr in r1["rows"][: len(r1["rows"]) - r1["n_in"]]:
        if not Cr:
            z.append(rnd.randint(0, 1))
        else:
            z.append(sum(c * z[v] for v, c in A) * sum(c * z[v] for v, c in B) % R)
    return z


def test_two_slots_prove_from_one_handle_at_once(bzk, co):
    r1, params, _, _ = _proof_case(co, 2000)
    zs = [fr_bytes(_rewitness(r1, 100 + k)) for k in range(16)]
    assert _first_unsat(r1, _rewitness(r1, 100)) == -1
    ph = bzk.params_load(params)
    mh = bzk.r1cs_mats_load(_csr_abc(r1), r1["n_in"], r1["n_aux"])
    ctxs = [Bzk(0), Bzk(0)]
    slots = [c.params_slot(ph) for c in ctxs]
    try:
        want = [bzk.groth16_prove_witness(ph, mh, zs[k], *_rs(k)) for k in range(16)]
        assert len(set(want)) == 16
        got = [None] * 16

        def run(t):
            for k in range(8 * t, 8 * t + 8):
                got[k] = ctxs[t].groth16_prove_witness(slots[t], mh, zs[k], *_rs(k), check=(k % 2 == 1))

        th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert got == want
    finally:
        for c, sl in zip(ctxs, slots):
            c.params_free(sl)
            c.close()
        bzk.r1cs_mats_free(mh)
        bzk.params_free(ph)


def test_call_refusals_leave_the_context_proving(bzk, co):
    r1, params, zb, (az, bz, cz) = _proof_case(co, 100)
    r, s = _rs(9)
    n_vars, n_rows = len(r1["z"]), len(r1["rows"])
    ph = bzk.params_load(params)
    abc = _csr_abc(r1)
    mh = bzk.r1cs_mats_load(abc, r1["n_in"], r1["n_aux"])
    host_mh = L.r1cs_mats_load(abc, r1["n_in"], r1["n_aux"])                  # loaded with ctx = NULL
    other = synth_r1cs(60, seed=1)
    other_mh = bzk.r1cs_mats_load(_csr_abc(other), other["n_in"], other["n_aux"])  # another circuit shape than the params
    tall = dict(r1, rows=r1["rows"] + r1["rows"][:100])                        # the same variables, 203 rows > 2^7
    tall_mh = bzk.r1cs_mats_load(_csr_abc(tall), r1["n_in"], r1["n_aux"])
    dz = to_dev(zb)
    outs = [torch.full((128 * 32,), 0xFF, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    lib = bzk.lib
    proof = C.create_string_buffer(b"\xaa" * 387, 387)
    refused = [
        ("n_vars != the handle's", lambda: lib.bzk_groth16_prove_witness(bzk.h, ph, mh, zb, n_vars - 1, r, s, 0, proof)),
        ("n_vars != the params'", lambda: lib.bzk_groth16_prove_witness(bzk.h, ph, other_mh, fr_bytes(other["z"]), len(other["z"]), r, s, 0, proof)),
        ("n_rows > 2^log_m", lambda: lib.bzk_groth16_prove_witness(bzk.h, ph, tall_mh, zb, n_vars, r, s, 0, proof)),
        ("a handle loaded with NULL", lambda: lib.bzk_groth16_prove_witness(bzk.h, ph, host_mh, zb, n_vars, r, s, 0, proof)),
        ("a NULL z", lambda: lib.bzk_groth16_prove_witness(bzk.h, ph, mh, None, n_vars, r, s, 0, proof)),
        ("eval_dev: n_vars", lambda: lib.bzk_r1cs_eval_dev(bzk.h, mh, dz.data_ptr(), n_vars + 1, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 128)),
        ("eval_dev: pad_rows < n_rows", lambda: lib.bzk_r1cs_eval_dev(bzk.h, mh, dz.data_ptr(), n_vars, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), n_rows - 1)),
        ("eval_dev: a handle loaded with NULL", lambda: lib.bzk_r1cs_eval_dev(bzk.h, host_mh, dz.data_ptr(), n_vars, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 128)),
        ("eval_dev: a NULL z", lambda: lib.bzk_r1cs_eval_dev(bzk.h, mh, None, n_vars, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 128)),
        ("eval: a handle loaded with NULL", lambda: lib.bzk_r1cs_eval(bzk.h, host_mh, zb, n_vars, None, None, None, None)),
        ("eval: n_vars", lambda: lib.bzk_r1cs_eval(bzk.h, mh, zb, n_vars - 1, None, None, None, None)),
        ("eval on host threads: a device handle", lambda: lib.bzk_r1cs_eval(None, mh, zb, n_vars, None, None, None, None)),
    ]
    try:
        for name, call in refused:
            assert call() == -1, name
        bzk.sync()
        assert proof.raw == b"\xaa" * 387 and all(dev_bytes(o) == b"\xff" * (128 * 32) for o in outs)  # nothing was launched
        want = co.groth16_prove(params, zb, az, bz, cz, r, s, nthreads=co.ncpu())
        assert bzk.groth16_prove_witness(ph, mh, zb, r, s) == want                  # a good proof follows on the same context
        assert bzk.groth16_prove(ph, zb, az, bz, cz, r, s) == want
    finally:
        for h in (mh, other_mh, tall_mh):
            bzk.r1cs_mats_free(h)
        L.r1cs_mats_free(host_mh)
        bzk.params_free(ph)
