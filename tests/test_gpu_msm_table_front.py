"""GPU parity of the passes a table call's partition front runs (bazuka_amd/csrc/msm_impl.cuh section 3d: msm_front_scatter_kernel<true> staging tile-local
32-bit words four levels a round, msm_front_table_bins_kernel ranking by (bucket, level) cells) against the CPU oracle's bytes, at the smallest shapes the new
arithmetic can break at.  One handle, a context under BZK_MSM_FRONT=partition and one under =sort.  Windows 12, 15, 19 and 20 have 22, 18, 14 and 13 levels: the
last round of four is partial in each, c = 15 fills the bin pass's counters, c = 20 is the default's.  At every window: n = 4097 and 8193 (more than one tile,
no multiple of it), the seven mixes of tests/test_gpu_msm_bases_table.py, a one-bucket mix (the same small digit in every window of every scalar: one bin, one
cell per level, holds every pair of the call), and a prefix of n - 1000.  At c = 20, n = 65 537 with the equal and half-equal mixes puts more than 2^16 values
into one (bucket, level) cell.  The bin pass has a capacity - front_table_bin_cap: the values it orders in LDS behind the cells - and a chunk - the
FRONT_TABLE_BIN_THREADS x FRONT_TABLE_BIN_UNROLL values a workgroup loads per step of a sweep over a fuller bin: bins of exactly the capacity, resp. a whole
number of chunks beyond it, one value fewer and one more are built from one-bucket scalars.  The order inside a bucket cannot be seen through
result bytes: tests/host/msm_front_table_check.hip proves it for the arithmetic."""
import os
import re

import pytest
import torch

from oracle import pyref as pr
from util import fr_bytes, fr_list, rand_scalars_bytes, to_dev

pytestmark = pytest.mark.gpu
R = pr.R_MOD
CS = [12, 15, 19, 20]
SIZES = [4097, 8193]
MIXES = ["uniform", "zero", "equal", "r-1", "carry", "small", "half-equal", "one-bucket"]
N_MAX = (1 << 16) + 1
MARK = "msm_bases_table"
FRONT = {"msm_digits", "msm_front_scan", "msm_front_scatter", "msm_front_bins"}
KNOBS = ("BZK_MSM_BASES_TABLE", "BZK_MSM_BASES_TABLE_C", "BZK_MSM_C", "BZK_MSM_FRONT", "BZK_MSM_SPLIT", "BZK_MSM_SPLIT_MIN_LOG", "BZK_MSM_SPLIT_PRIO",
         "BZK_MSM_SPLIT_CUTS")


def _front_constant(name):
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bazuka_amd", "csrc", "msm_front.cuh")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


THREADS, HELD, LDS_WORDS = (_front_constant("FRONT_TABLE_" + k) for k in ("BIN_THREADS", "BIN_HELD", "LDS_WORDS"))
CHUNK = THREADS * _front_constant("FRONT_TABLE_BIN_UNROLL")


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
    """contexts by (table window, BZK_MSM_FRONT), created on first use, closed with the module"""
    made = {}

    def get(c, front):
        if (c, front) not in made:
            made[(c, front)] = _ctx_with_env({"BZK_MSM_BASES_TABLE": "1", "BZK_MSM_BASES_TABLE_C": str(c), "BZK_MSM_FRONT": front})
        return made[(c, front)]

    yield get
    for ctx in made.values():
        ctx.close()


def _digit_windows(c, d, windows):
    """the scalar whose raw digit is d in the lowest `windows` windows and zero above"""
    return sum(d << (c * w) for w in range(windows)) % R


def scalars(mix, n, c):
    """Montgomery-form scalar bytes of the mix (deterministic)"""
    if mix == "uniform":
        return rand_scalars_bytes(n, 1000 + n)
    if mix == "zero":
        return bytes(32 * n)
    if mix == "equal":
        return pr.fr_to_mont_bytes(fr_list(1, 77)[0]) * n
    if mix == "r-1":
        return pr.fr_to_mont_bytes(R - 1) * n
    if mix == "carry":
        a, b = (pr.fr_to_mont_bytes(_digit_windows(c, d, 253 // c)) for d in ((1 << (c - 1)), (1 << (c - 1)) + 1))
        return ((a + b) * (n // 2 + 1))[:32 * n]
    if mix == "small":
        rng = pr.SplitMix64(5 + n)
        return fr_bytes([rng.fr() % (1 << 44) for _ in range(n)])
    if mix == "one-bucket":
        return pr.fr_to_mont_bytes(_digit_windows(c, 5, 253 // c)) * n
    assert mix == "half-equal"
    return pr.fr_to_mont_bytes(fr_list(1, 78)[0]) * (n // 2) + rand_scalars_bytes(n - n // 2, 2000 + n)


_bases, _want = {}, {}


def bases_of(co, n):
    """host bytes of the first n points of one seeded set (a prefix of a set is a set)"""
    if "g1" not in _bases:
        _bases["g1"] = co.g1_bases(4343, 0, N_MAX, nthreads=co.ncpu())
    return _bases["g1"][:n * 96]


def want_of(co, n, scb, tag):
    """the oracle's result, computed once per input and shared by every window and front"""
    if (n, tag) not in _want:
        _want[(n, tag)] = co.msm_g1(bases_of(co, n), scb, nthreads=co.ncpu())
    return _want[(n, tag)]


def _tag(mix, c):
    return (mix, c if mix in ("carry", "one-bucket") else 0)


class Loaded:
    """a resident set of the first n points on `ctx`, freed on exit"""

    def __init__(self, co, ctx, n):
        self.ctx, self.n = ctx, n
        self.db = to_dev(bases_of(co, n))
        torch.cuda.synchronize()

    def __enter__(self):
        self.h = self.ctx.msm_bases_load_dev(self.db, self.n)
        return self.h

    def __exit__(self, *exc):
        self.ctx.msm_bases_free(self.h)


def _both(co, part, sort, h, scb, m, tag, what):
    sc = to_dev(scb)
    torch.cuda.synchronize()
    want = want_of(co, m, scb, tag)
    assert part.msm_bases_run_dev(h, sc, m) == want, ("partition",) + what
    assert sort.msm_bases_run_dev(h, sc, m) == want, ("sort",) + what


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", CS)
def test_every_mix_through_both_fronts(co, ctxs, c, n):
    part, sort = ctxs(c, "partition"), ctxs(c, "sort")
    with Loaded(co, part, n) as h:
        assert part.msm_bases_table_info(h)["levels"] == (256 + c - 1) // c
        for mix in MIXES:
            _both(co, part, sort, h, scalars(mix, n, c), n, _tag(mix, c), (c, n, mix))
        m = n - 1000  # a prefix: the table's stride stays the set's
        for mix in ("half-equal", "one-bucket"):
            _both(co, part, sort, h, scalars(mix, m, c), m, _tag(mix, c), (c, n, mix, "prefix"))


@pytest.mark.parametrize("mix", ["equal", "half-equal"])
def test_a_cell_beyond_sixteen_bits(co, ctxs, mix):
    """n = 2^16 + 1 equal scalars at c = 20: every level's (bucket, level) cell holds more values than a 16-bit counter counts"""
    c, n = 20, N_MAX
    part, sort = ctxs(c, "partition"), ctxs(c, "sort")
    with Loaded(co, part, n) as h:
        _both(co, part, sort, h, scalars(mix, n, c), n, _tag(mix, c), (c, n, mix))


def _stage_cap(c):
    """front_table_bin_cap of a whole call at window c: the values that fit behind the (bucket, level) cells, and in the lanes' registers"""
    cells = ((256 + c - 1) // c) << min(10, c - 5)
    return min(LDS_WORDS - cells, HELD * THREADS)


@pytest.mark.parametrize("c", CS)
def test_a_bin_around_the_stage_and_around_a_chunk_of_the_sweeps(co, ctxs, c):
    """one bin of exactly the stage's capacity, one value fewer and one more (ordered in LDS, resp. stored through the cursors), and of a whole number of the
    sweeps' chunks beyond it, one fewer and one more: k scalars with the digit in every window, one more with it in the lowest r windows"""
    per = 253 // c
    cap = _stage_cap(c)
    whole = (cap + 1) // CHUNK * CHUNK + CHUNK
    counts = (cap - 1, cap, cap + 1, whole - 1, whole, whole + 1)
    part, sort = ctxs(c, "partition"), ctxs(c, "sort")
    n = counts[-1] // per + 1
    with Loaded(co, part, n) as h:
        for cnt in counts:
            k, r = divmod(cnt, per)
            scb = pr.fr_to_mont_bytes(_digit_windows(c, 5, per)) * k + pr.fr_to_mont_bytes(_digit_windows(c, 5, r)) + bytes(32 * (n - k - 1))
            _both(co, part, sort, h, scb, n, ("bin of", c, cnt), (c, cnt))


@pytest.mark.parametrize("c", CS)
def test_the_partition_call_runs_the_four_passes(co, ctxs, c):
    """no silent fall-back at any of the windows: the partition context's table call shows msm_digits and the three passes behind it and no pair sort"""
    n = SIZES[0]
    part = ctxs(c, "partition")
    scb = scalars("uniform", n, c)
    sc = to_dev(scb)
    torch.cuda.synchronize()
    with Loaded(co, part, n) as h:
        part.prof_enable(True)
        part.prof_reset()
        try:
            got = part.msm_bases_run_dev(h, sc, n)
            p = part.prof_dump()
        finally:
            part.prof_enable(False)
    assert got == want_of(co, n, scb, ("uniform", 0))
    assert FRONT | {MARK} <= set(p) and "msm_sort_pairs" not in p and "msm_offsets" not in p, sorted(p)
    assert p["msm_accumulate"][0] == 1, p
