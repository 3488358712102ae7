"""The host code of the witness-only evaluation (bazuka_amd/csrc/bzk_r1cs_eval.cuh) on the CPU: tests/host/r1cs_eval_check.hip is built by build() with
the address and undefined-behaviour sanitizers and BZK_FP28_CHECK - the column assertions of wide_mac and wide_reduce are live - and runs as a child process.
The table of tests/r1cs_eval_cases.py (rows of 0, 1, 5, 6, 7, 11, 12, 13, 63, 64, 65, 255, 256, 257 and 1000 terms, each with every coefficient and value
r - 1, every coefficient r - 2 on values r - 1, every coefficient 1, and a seeded mixture; a repeated column, a stored zero, column 0 and the last column)
goes to the program as a file; it evaluates every row through row_eval, through the kernel's wave schedule and through chunks cut from the other end, and
the bytes it returns are compared with Python integers.  The program also runs the loader's validation over every malformed matrix of the refusal list,
each array in a heap block of exactly its size."""
import os
import struct
import subprocess

import pytest

import r1cs_eval_cases as cases
from oracle import pyref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "host", "_r1cs_eval_check")


def _run(args):
    assert os.path.exists(EXE), "tests/host/_r1cs_eval_check not built (build() compiles it)"
    p = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return p.stdout


def _evaluate(tmp_path, rows, z):
    n_rows, rp, col, val = cases.csr_bytes(rows)
    src, dst = tmp_path / "table.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<3Q", len(z), n_rows, len(col) // 4) + rp + col + val + b"".join(pr.fr_to_mont_bytes(v) for v in z))
    out = _run(["table", str(src), str(dst)])
    assert "table holds" in out
    got = dst.read_bytes()
    assert len(got) == 32 * n_rows
    return [got[32 * i:32 * i + 32] for i in range(n_rows)]


def test_structured_table_matches_python_integers(tmp_path):
    z, tab = cases.witness(), cases.table()
    assert len(tab) == 4 * len(cases.LENGTHS) + 6
    rows = [r for _, r in tab]
    got = _evaluate(tmp_path, rows, z)
    want = cases.expected(rows, z)
    for (name, _), g, w in zip(tab, got, want):
        assert g == pr.fr_to_mont_bytes(w), name


def test_a_witness_whose_limbs_are_not_a_residue_is_evaluated_inside_the_arrays(tmp_path):
    """z is taken as canonical, an entry >= r is not refused: the bound of the chunk (k 3 per operand) covers 2^256 - 1, so the column assertions stay
    quiet and the result is the residue of the same sum - and the sanitizer sees every read"""
    rows = [[(1 + (k % 3), pr.R_MOD - 1) for k in range(n)] for n in (1, 6, 7, 64, 385)]
    src, dst = tmp_path / "t.bin", tmp_path / "o.bin"
    n_rows, rp, col, val = cases.csr_bytes(rows)
    raw = [1, (1 << 256) - 1, pr.R_MOD, pr.R_MOD + 12345]  # limbs as they are: no reduction on the way in
    mont_inv = pow(1 << 256, -1, pr.R_MOD)
    zb = pr.fr_to_mont_bytes(1) + b"".join(v.to_bytes(32, "little") for v in raw[1:])
    src.write_bytes(struct.pack("<3Q", 4, n_rows, len(col) // 4) + rp + col + val + zb)
    assert "table holds" in _run(["table", str(src), str(dst)])
    got = dst.read_bytes()
    zval = [1] + [v * mont_inv % pr.R_MOD for v in raw[1:]]  # what those limbs stand for
    for i, w in enumerate(cases.expected(rows, zval)):
        assert got[32 * i:32 * i + 32] == pr.fr_to_mont_bytes(w), i


def test_loader_validation_refuses_every_malformed_matrix():
    out = _run(["refusals"])
    assert "refusals hold" in out and int(out.split()[0]) >= 16
