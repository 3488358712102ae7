"""GPU parity on structured and top-of-range values (tests/fr_value_cases.py): the NTT, the fused h chain, the Poseidon batch and the 4-ary tree against
the CPU oracle, bit-exact.

Every other GPU input of these kernels comes from rand_scalars_bytes, whose raw limbs stay below 2^254: the 45 % of the field above it (the largest top
29-bit limb) and residue 0 as an operand (a product of a non-zero multiple of r comes out as exactly r; the final store's t == r case) are only met here.
Expected bytes are the oracle's (co.ntt, co.groth16_h, co.poseidon_batch, co.merkle4_root) or a closed form, never the library's."""
import numpy as np
import pytest
import torch

import fr_value_cases as V
from fr_value_cases import raw_fr_bytes
from util import dev_bytes, fr_bytes, to_dev

pytestmark = pytest.mark.gpu

MODES = ((False, False), (False, True), (True, False), (True, True))  # (inverse, coset)
SMALL = tuple(range(1, 13))      # 1 .. 10 one pass (odd and even stage counts, up to the full ten), 11 and 12 two passes 6+5, 6+6
LARGE = (19, 20, 21)             # 10+9, 10+10 and 7+7+7 (the single-level table of the second boundary)


def _first_diff(got, want):
    """index of the first 32-byte element that differs, or None"""
    assert len(got) == len(want), (len(got), len(want))
    if got == want:
        return None
    d = (np.frombuffer(got, dtype=np.uint8).reshape(-1, 32) != np.frombuffer(want, dtype=np.uint8).reshape(-1, 32)).any(axis=1)
    return int(np.argmax(d))


_slot = {}


def _cached(kind, n, make):
    """one slot per kind: the cases of one size follow each other, and the large vectors are not kept beyond them"""
    if _slot.get(kind, (None, None))[0] != n:
        _slot[kind] = (n, make())
    return _slot[kind][1]


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_vectors():
    yield
    _slot.clear()


def _patterns(n, which=None):
    return _cached(("ntt", which), n, lambda: [(name, raw_fr_bytes(v)) for name, v in V.named(n, which)])


def _ntt_cases():
    out = [pytest.param(lg, inv, cs, None, id="%d-inv%d-coset%d" % (lg, inv, cs)) for lg in SMALL for inv, cs in MODES]
    out += [pytest.param(lg, inv, cs, p, id="%d-inv%d-coset%d-%s" % (lg, inv, cs, p)) for lg in LARGE for p in V.LARGE for inv, cs in MODES]
    return out


@pytest.mark.parametrize("log_n,inv,cs,only", _ntt_cases())
def test_ntt_patterns_vs_oracle(bzk, co, log_n, inv, cs, only):
    """every pattern up to 2^12; zeros, top, sparse and delta(n - 1) from 2^19 on (one pattern per case there)"""
    n = 1 << log_n
    cases = _patterns(n) if only is None else [c for c in _patterns(n, V.LARGE) if c[0] == ("delta(%d)" % (n - 1) if only == "delta(n-1)" else only)]
    assert cases
    for name, data in cases:
        got = bzk.ntt(data, log_n, inv, cs)
        want = co.ntt(data, log_n, inv, cs, nthreads=co.ncpu())
        assert got == want, "pattern %s, n 2^%d, inverse %d coset %d: first differing element %s" % (name, log_n, inv, cs, _first_diff(got, want))
        if name == "zeros":  # the t == r case of the final store's conditional subtraction at every output
            assert got == bytes(32 * n), "zeros, n 2^%d, inverse %d coset %d: first non-zero element %s" % (log_n, inv, cs, _first_diff(got, bytes(32 * n)))


@pytest.mark.parametrize("cs", [False, True])
@pytest.mark.parametrize("log_n", SMALL + LARGE)
def test_ntt_top_roundtrip(bzk, log_n, cs):
    n = 1 << log_n
    data = dict(_patterns(n, V.LARGE if log_n in LARGE else None))["top"]
    d = to_dev(data)
    torch.cuda.synchronize()
    bzk.ntt_dev(d, log_n, False, cs)
    bzk.ntt_dev(d, log_n, True, cs)
    bzk.sync()
    got = dev_bytes(d)
    assert got == data, "top round trip, n 2^%d, coset %d: first differing element %s" % (log_n, cs, _first_diff(got, data))


@pytest.mark.parametrize("log_n", range(1, 7))
def test_ntt_top_vs_python_reference(bzk, pr, log_n):
    n = 1 << log_n
    raw = V.top(n)
    vals = [pr.fr_from_mont_bytes(v.to_bytes(32, "little")) for v in raw]
    for inv, cs in MODES:
        got = bzk.ntt(raw_fr_bytes(raw), log_n, inv, cs)
        want = fr_bytes(pr.ntt(vals, log_n, inv, cs))
        assert got == want, "top vs pyref, n 2^%d, inverse %d coset %d: first differing element %s" % (log_n, inv, cs, _first_diff(got, want))


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("log_m", [1, 2, 5, 10, 11, 12, 20])
def test_h_chain_cases_vs_oracle(bzk, co, log_m, case):
    """zeros ; three independent top vectors, no padding ; constant r - 1 with c = a b (A B - C the zero polynomial) ; top with c = a b (a real proof's
    case: A B - C vanishes on the domain) ; top with c = 0 ; one row"""
    m = 1 << log_m
    name, a, b, c, zero = _cached("h", m, lambda: V.h_cases(m))[case]
    az, bz, cz = raw_fr_bytes(a), raw_fr_bytes(b), raw_fr_bytes(c)
    pad = bytes(32 * (m - len(a)))
    da, db, dc = to_dev(az + pad), to_dev(bz + pad), to_dev(cz + pad)
    torch.cuda.synchronize()
    bzk.groth16_h_dev(da, db, dc, log_m)
    bzk.sync()
    got = dev_bytes(da)[: 32 * (m - 1)]
    want = co.groth16_h(az, bz, cz, log_m, nthreads=co.ncpu())
    assert got == want, "h case %s, m 2^%d, %d rows: first differing coefficient %s" % (name, log_m, len(a), _first_diff(got, want))
    if zero:
        assert got == bytes(32 * (m - 1)), "h case %s, m 2^%d: first non-zero coefficient %s" % (name, log_m, _first_diff(got, bytes(32 * (m - 1))))


POSEIDON_PATTERNS = ("zeros", "const_rm1", "top", "limbs")


@pytest.mark.parametrize("n", [1, 9, 8192, 8193])
@pytest.mark.parametrize("arity", [1, 2, 3, 4, 5, 6, 7, 16])
def test_poseidon_batch_patterns_vs_oracle(bzk, co, arity, n):
    """both sides of the cooperative / one-lane-per-hash switch at 8192 hashes, width 5's own kernel, the 32-bit-limb kernel of the wide arity"""
    for name, vals in V.named(n * arity, POSEIDON_PATTERNS):
        inp = raw_fr_bytes(vals)
        got = bzk.poseidon_batch(inp, arity)
        want = co.poseidon_batch(inp, arity, nthreads=co.ncpu())
        assert got == want, "pattern %s, arity %d, %d hashes: first differing hash %s" % (name, arity, n, _first_diff(got, want))


@pytest.mark.parametrize("log4", [1, 5])
@pytest.mark.parametrize("pattern", ["top", "const_rm1"])
def test_merkle4_patterns_vs_oracle(bzk, co, pattern, log4):
    (name, vals), = V.named(4 ** log4, (pattern,))
    leaves = raw_fr_bytes(vals)
    root, nodes = bzk.merkle4_root(leaves, log4, want_nodes=True)
    oroot, onodes = co.merkle4_root(leaves, log4, True, nthreads=co.ncpu())
    assert root == oroot, "pattern %s, 4^%d leaves: root" % (name, log4)
    assert nodes == onodes, "pattern %s, 4^%d leaves: first differing node %s" % (name, log4, _first_diff(nodes, onodes))
