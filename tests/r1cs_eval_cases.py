"""The structured table of the witness-only evaluation's tests (tests/test_r1cs_eval_cpu.py on the host code, tests/test_gpu_r1cs_eval.py on the kernel):
rows whose lengths sit on both sides of every cut the code makes - the 6-term chunk (5, 6, 7, 11, 12, 13), the lane / wave split at 12 terms (12, 13),
the 64 lanes of a wave times one chunk and the wave's second round (63, 64, 65, 255, 256, 257 terms; 1000 terms = 167 chunks) - each with operands at the
top of the range, and the entries a loader must take as they are: a repeated column, a stored zero, column 0 and the last column.  Everything is Python
integers; expected() is the definition of the result."""
import random
import struct

from oracle import pyref as pr

R = pr.R_MOD
LENGTHS = (0, 1, 5, 6, 7, 11, 12, 13, 63, 64, 65, 255, 256, 257, 1000)
N_TOP, N_RAND = 1000, 1000  # variables 1 .. 1000 hold r - 1, the next 1000 seeded values; variable 0 is ONE, the last one seeded


def witness(seed=20260101):
    rnd = random.Random(seed)
    return [1] + [R - 1] * N_TOP + [rnd.randrange(R) for _ in range(N_RAND)] + [rnd.randrange(1, R)]


def table(seed=20260102):
    """[(name, [(column, coefficient)])]: 15 lengths x 4 fillings, longest first, then the special rows"""
    rnd = random.Random(seed)
    n_vars = 1 + N_TOP + N_RAND + 1
    rows = []
    for n in sorted(LENGTHS, reverse=True):
        top_cols = [1 + (k % N_TOP) for k in range(n)]                     # every value r - 1, no column twice
        rows.append((f"{n} terms, coefficients and values r - 1", [(c, R - 1) for c in top_cols]))
        rows.append((f"{n} terms, coefficients r - 2, values r - 1", [(c, R - 2) for c in top_cols]))
        rows.append((f"{n} terms, coefficients 1", [(1 + N_TOP + (k % N_RAND), 1) for k in range(n)]))
        mix = []
        for k in range(n):
            coeff = rnd.choice((1, 1, R - 1, R - 1, R - 2, 2, 1 << 64, 1 << 254, rnd.randrange(R), rnd.randrange(R)))
            mix.append((rnd.choice((0, n_vars - 1, rnd.randrange(n_vars), rnd.randrange(n_vars), 1 + rnd.randrange(N_TOP))), coeff))
        rows.append((f"{n} terms, seeded mixture", mix))
    v = 1 + N_TOP + 5
    rows.append(("one column three times", [(v, 3), (v, R - 5), (v, rnd.randrange(R))]))
    rows.append(("one column 14 times across three chunks", [(v + 1, 1 + k) for k in range(14)]))
    rows.append(("a stored zero beside a term", [(v + 2, 0), (v + 3, 7)]))
    rows.append(("a stored zero alone", [(2, 0)]))
    rows.append(("column 0 and the last column", [(0, R - 3), (n_vars - 1, rnd.randrange(R))]))
    rows.append(("the last column alone, coefficient r - 1", [(n_vars - 1, R - 1)]))
    return rows


def expected(rows, z):
    return [sum(c * z[v] for v, c in row) % R for row in rows]


def csr_bytes(rows):
    """(n_rows, row_ptr bytes, col bytes, val bytes) as Bzk.groth16_setup / r1cs_mats_load take a matrix"""
    rp, col, val = [0], [], []
    for row in rows:
        for v, c in row:
            col.append(v)
            val.append(pr.fr_to_mont_bytes(c))
        rp.append(len(col))
    return (len(rows), struct.pack(f"<{len(rp)}I", *rp), struct.pack(f"<{len(col)}I", *col), b"".join(val))


def triple(n_rows):
    """three different matrices of n_rows rows over the table's witness: A takes the table's rows in order (cycling), B and C start further in"""
    rows = [r for _, r in table()]
    return [[rows[(i + shift) % len(rows)] for i in range(n_rows)] for shift in (0, 17, 41)]
