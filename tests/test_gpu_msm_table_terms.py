"""GPU parity of the PLAIN term layout a table call over a resident G1 set leaves its one bucket set's terms in (bazuka_amd/csrc/msm_impl.cuh
msm_bitsum_quad_kernel<128, true>: one 256-lane tree per bit, the host's Horner adding a term at every bit).  Contexts as tests/test_gpu_msm_table_front.py makes
them - BZK_MSM_BASES_TABLE=1 and BZK_MSM_BASES_TABLE_C = 11, 12, 16, 19, 20 (both parities of c - 1; c = 20 has column bits of 512 leaves: two per lane) -, one per
window in the default layout and one under BZK_MSM_BITSUM_PLAIN=0 (the paired layout of every other caller).  At n = 1, 2, 3, 2^10, 2^12 every result of
msm_bases_run_dev must equal msm_g1_dev on the raw bases and the CPU oracle's bytes.  Scalars: uniform, all zero, all equal (one bucket per level holds every
entry), all r - 1, the front test's carry mix, every digit 2^(c-1) at one level (the top bucket and the carry), and `runs`: entries 0, 1, 4 and entries 2, 3, 5
share a scalar of their own, so that a run STARTS with them.  Base arrays: a seeded set; `twins` (point 1 = point 0, point 3 = -point 2) and `mirror` (point 1 =
-point 0, point 3 = point 2) put a repeated point and a point with its negative at the head of a run - the doubling and the cancellation branch of a run's second
addition, with a third entry behind them; at n = 2 with equal scalars `mirror` sums to the identity: every term of the set is one."""
import os

import pytest
import torch

from oracle import pyref as pr
from util import fr_list, rand_scalars_bytes, to_dev

pytestmark = pytest.mark.gpu
R = pr.R_MOD
P_MOD = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
CS = [11, 12, 16, 19, 20]
SIZES = [1, 2, 3, 1 << 10, 1 << 12]
N_MAX = SIZES[-1]
MIXES = ["uniform", "zero", "equal", "r-1", "carry", "top", "runs"]
ARRAYS = {"set": MIXES, "twins": ["equal", "runs"], "mirror": ["equal", "runs"]}
MARK = "msm_bases_table"
KNOBS = ("BZK_MSM_BASES_TABLE", "BZK_MSM_BASES_TABLE_C", "BZK_MSM_C", "BZK_MSM_FRONT", "BZK_MSM_SPLIT", "BZK_MSM_SPLIT_MIN_LOG", "BZK_MSM_SPLIT_PRIO",
         "BZK_MSM_SPLIT_CUTS", "BZK_MSM_BITSUM_PLAIN")


def _ctx_with_env(env):
    """a context of its own created under exactly `env` among the MSM knobs (they are read when a context is created)"""
    from bazuka_amd import Bzk
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        return Bzk(0)
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


@pytest.fixture(scope="module")
def ctxs():
    """contexts by (table window, layout), created on first use, closed with the module"""
    made = {}

    def get(c, layout):
        if (c, layout) not in made:
            env = {"BZK_MSM_BASES_TABLE": "1", "BZK_MSM_BASES_TABLE_C": str(c)}
            if layout == "paired":
                env["BZK_MSM_BITSUM_PLAIN"] = "0"
            made[(c, layout)] = _ctx_with_env(env)
        return made[(c, layout)]

    yield get
    for ctx in made.values():
        ctx.close()


def _neg(rec):
    """the raw record of -P: y -> p - y (Montgomery residues negate like any other)"""
    y = int.from_bytes(rec[48:96], "little")
    return rec[:48] + ((P_MOD - y) % P_MOD).to_bytes(48, "little")


_seeded, _want = {}, {}


def bases_of(co, arr, n):
    if "set" not in _seeded:
        _seeded["set"] = co.g1_bases(5151, 0, N_MAX, nthreads=co.ncpu())
    rec = [_seeded["set"][96 * i:96 * i + 96] for i in range(min(n, 4))]
    if arr != "set" and n >= 2:
        rec[1] = rec[0] if arr == "twins" else _neg(rec[0])
    if arr != "set" and n >= 4:
        rec[3] = _neg(rec[2]) if arr == "twins" else rec[2]
    return b"".join(rec) + _seeded["set"][96 * len(rec):96 * n]


def scalars(mix, n, c):
    """Montgomery-form scalar bytes of the mix (deterministic)"""
    if mix == "uniform":
        return rand_scalars_bytes(n, 3000 + n)
    if mix == "zero":
        return bytes(32 * n)
    if mix == "equal":
        return pr.fr_to_mont_bytes(fr_list(1, 79)[0]) * n
    if mix == "r-1":
        return pr.fr_to_mont_bytes(R - 1) * n
    if mix == "carry":
        per = 253 // c
        a, b = (pr.fr_to_mont_bytes(sum(d << (c * w) for w in range(per)) % R) for d in ((1 << (c - 1)), (1 << (c - 1)) + 1))
        return ((a + b) * (n // 2 + 1))[:32 * n]
    if mix == "top":
        return pr.fr_to_mont_bytes((1 << (c - 1)) << c) * n   # every digit of level 1 is 2^(c-1)
    assert mix == "runs"
    sa, sb = (pr.fr_to_mont_bytes(v) for v in fr_list(2, 80))
    u = rand_scalars_bytes(n, 4000 + n)
    head = b"".join((sa, sa, sb, sb, sa, sb)[:n])
    return head + u[len(head):]


def want_of(co, arr, n, mix, c, bb, scb):
    """the oracle's bytes, computed once per input and shared by every window and layout"""
    key = (arr, n, mix, c if mix in ("carry", "top") else 0)
    if key not in _want:
        _want[key] = co.msm_g1(bb, scb, nthreads=co.ncpu())
    return _want[key]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", CS)
def test_table_calls_in_both_layouts_equal_the_plain_call_and_the_oracle(co, ctxs, c, n):
    plain, paired = ctxs(c, "plain"), ctxs(c, "paired")
    for arr, mixes in ARRAYS.items():
        bb = bases_of(co, arr, n)
        db = to_dev(bb)
        torch.cuda.synchronize()
        hs = [(ctx, ctx.msm_bases_load_dev(db, n)) for ctx in (plain, paired)]
        try:
            for ctx, h in hs:
                assert ctx.msm_bases_table_info(h) == {"c": c, "levels": (256 + c - 1) // c, "table_bytes": ((256 + c - 1) // c) * n * 112}
            for mix in mixes:
                scb = scalars(mix, n, c)
                sc = to_dev(scb)
                torch.cuda.synchronize()
                want = want_of(co, arr, n, mix, c, bb, scb)
                assert plain.msm_g1_dev(db, sc, n) == want, ("raw bases", c, n, arr, mix)
                for (ctx, h), layout in zip(hs, ("plain", "paired")):
                    assert ctx.msm_bases_run_dev(h, sc, n) == want, (layout, c, n, arr, mix)
        finally:
            for ctx, h in hs:
                ctx.msm_bases_free(h)


@pytest.mark.parametrize("layout", ["plain", "paired"])
def test_the_table_call_runs_one_bit_sum_launch(co, ctxs, layout):
    """no fall-back in either layout: the call is the table's (its label), with one msm_rowcol and one msm_bitsum launch and no window-sum kernel behind them"""
    c, n = 20, N_MAX
    ctx = ctxs(c, layout)
    bb, scb = bases_of(co, "set", n), scalars("uniform", n, c)
    db, sc = to_dev(bb), to_dev(scb)
    torch.cuda.synchronize()
    h = ctx.msm_bases_load_dev(db, n)
    try:
        ctx.prof_enable(True)
        ctx.prof_reset()
        try:
            got = ctx.msm_bases_run_dev(h, sc, n)
            p = ctx.prof_dump()
        finally:
            ctx.prof_enable(False)
    finally:
        ctx.msm_bases_free(h)
    assert got == want_of(co, "set", n, "uniform", c, bb, scb)
    assert MARK in p and p["msm_bitsum"][0] == 1 and p["msm_rowcol"][0] == 1 and p["msm_accumulate"][0] == 1, sorted(p)
