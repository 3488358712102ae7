"""GPU parity of the window table a resident G1 base set may carry (bazuka_amd/csrc/msm_impl.cuh msm_bases_table_plan, msm_bases_entry): a set loaded on a
context created under BZK_MSM_BASES_TABLE=1 owns a full static table with the window BZK_MSM_BASES_TABLE_C, and a whole stand-alone call over it runs from that
table.  With windows 11, 16 and 20 such calls must return the CPU oracle's bytes for set sizes around the tile and workgroup boundaries of every pass and for
scalar vectors that empty, fill or overflow single buckets, for a prefix of the set and for canonical input; a throughput-flagged call, a de-duplicated call
and a window range over the same handle must return the same bytes from the per-call pipeline; the launch labels must say which path ran; the handle must report
the table's bytes; the sets a Groth16 parameter set loads for itself must carry no table; and contexts created under BZK_MSM_FRONT=partition and =sort must
bucket the table call's pairs by the partition passes resp. the pair sort, with the oracle's bytes either way."""
import os

import pytest
import torch

from oracle import pyref as pr
from util import fr_bytes, fr_list, r1cs_to_csr, rand_scalars_bytes, synth_r1cs, to_dev

pytestmark = pytest.mark.gpu
R = pr.R_MOD
SIZES = [1, 63, 4095, 4096, 4097, (1 << 13) + 1]
MIXES = ["uniform", "zero", "equal", "r-1", "carry", "small", "half-equal"]
CS = [11, 16, 20]
MARK = "msm_bases_table"  # the label only a call that runs from a set's table emits
KNOBS = ("BZK_MSM_BASES_TABLE", "BZK_MSM_BASES_TABLE_C", "BZK_MSM_C", "BZK_MSM_FRONT", "BZK_MSM_SPLIT", "BZK_MSM_SPLIT_MIN_LOG", "BZK_MSM_SPLIT_PRIO",
         "BZK_MSM_SPLIT_CUTS")


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
    """contexts by table window (0: BZK_MSM_BASES_TABLE=0, None: no knob at all) and BZK_MSM_FRONT, created on first use, closed with the module"""
    made = {}

    def get(c, front=None):
        if (c, front) not in made:
            env = {} if c is None else {"BZK_MSM_BASES_TABLE": "0"} if c == 0 else {"BZK_MSM_BASES_TABLE": "1", "BZK_MSM_BASES_TABLE_C": str(c)}
            if front:
                env["BZK_MSM_FRONT"] = front
            made[(c, front)] = _ctx_with_env(env)
        return made[(c, front)]

    yield get
    for ctx in made.values():
        ctx.close()


def _carry_values(c):
    """scalars whose raw digit is 2^(c-1) resp. 2^(c-1) + 1 in every window: the first stays positive, the second turns negative and carries"""
    return [sum(d << (c * w) for w in range(253 // c)) % R for d in ((1 << (c - 1)), (1 << (c - 1)) + 1)]


def scalars(mix, n, c):
    """Montgomery-form scalar bytes of the mix (deterministic): the mixes of tests/test_gpu_msm_front.py"""
    if mix == "uniform":
        return rand_scalars_bytes(n, 1000 + n)
    if mix == "zero":
        return bytes(32 * n)
    if mix == "equal":
        return pr.fr_to_mont_bytes(fr_list(1, 77)[0]) * n
    if mix == "r-1":
        return pr.fr_to_mont_bytes(R - 1) * n
    if mix == "carry":
        a, b = (pr.fr_to_mont_bytes(v) for v in _carry_values(c))
        return ((a + b) * (n // 2 + 1))[:32 * n]
    if mix == "small":
        rng = pr.SplitMix64(5 + n)
        return fr_bytes([rng.fr() % (1 << 44) for _ in range(n)])
    assert mix == "half-equal"
    return pr.fr_to_mont_bytes(fr_list(1, 78)[0]) * (n // 2) + rand_scalars_bytes(n - n // 2, 2000 + n)


_bases, _want = {}, {}


def bases_of(co, n):
    """host bytes of the first n points of one seeded set (a prefix of a set is a set)"""
    if "g1" not in _bases:
        _bases["g1"] = co.g1_bases(4343, 0, SIZES[-1], nthreads=co.ncpu())
    return _bases["g1"][:n * 96]


def want_of(co, n, scb, tag):
    """the oracle's result, computed once per input and shared by every window and call form"""
    key = (n, tag)
    if key not in _want:
        _want[key] = co.msm_g1(bases_of(co, n), scb, nthreads=co.ncpu())
    return _want[key]


def profiled(ctx, call):
    """(result, {label: (launches, ms)}) of one call"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        got = call()
        return got, ctx.prof_dump()
    finally:
        ctx.prof_enable(False)


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


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", CS)
def test_every_size_and_mix_from_the_table(co, ctxs, c, n):
    ctx = ctxs(c)
    with Loaded(co, ctx, n) as h:
        assert ctx.msm_bases_table_info(h)["c"] == c
        for mix in MIXES:
            scb = scalars(mix, n, c)
            sc = to_dev(scb)
            torch.cuda.synchronize()
            want = want_of(co, n, scb, (mix, c if mix == "carry" else 0))
            got, prof = profiled(ctx, lambda: ctx.msm_bases_run_dev(h, sc, n))
            assert got == want, (c, n, mix)
            assert MARK in prof, (c, n, mix, sorted(prof))


@pytest.mark.parametrize("c", CS)
def test_prefix_and_canonical_calls_on_the_same_handle(co, ctxs, c):
    """a prefix of the set gathers with the SET's stride; canonical input with values >= r is reduced before the recoding"""
    n = SIZES[-1]
    ctx = ctxs(c)
    with Loaded(co, ctx, n) as h:
        for m in (n - 1000, 1):
            scb = scalars("uniform", m, c)
            sc = to_dev(scb)
            torch.cuda.synchronize()
            got, prof = profiled(ctx, lambda: ctx.msm_bases_run_dev(h, sc, m))
            assert got == want_of(co, m, scb, ("uniform", 0)), (c, m)
            assert MARK in prof
        m = 4097
        can = [R + 5, 2 * R + 1, (1 << 256) - 1, R, 7, 0] + fr_list(m - 6, 31)
        scc = to_dev(b"".join(v.to_bytes(32, "little") for v in can))
        torch.cuda.synchronize()
        got, prof = profiled(ctx, lambda: ctx.msm_bases_run_dev(h, scc, m, canonical=True))
        assert got == want_of(co, m, fr_bytes([v % R for v in can]), ("canonical", 0)), c
        assert MARK in prof


@pytest.mark.parametrize("c", CS)
def test_other_call_forms_fall_back_with_the_same_bytes(co, ctxs, c):
    """throughput-flagged and de-duplicated calls and window ranges over a handle that owns a table keep the per-call pipeline: same bytes, no marker"""
    n = SIZES[-1]
    ctx = ctxs(c)
    with Loaded(co, ctx, n) as h:
        for mix in ("uniform", "half-equal"):
            scb = scalars(mix, n, c)
            sc = to_dev(scb)
            torch.cuda.synchronize()
            want = want_of(co, n, scb, (mix, 0))
            for form in ("throughput", "dedup"):
                got, prof = profiled(ctx, lambda: ctx.msm_bases_run_dev(h, sc, n, **{form: True}))
                assert got == want, (c, mix, form)
                assert MARK not in prof and prof.get("msm_accumulate", (0, 0.0))[0] >= 1, (c, mix, form, sorted(prof))
            W = ctx.msm_window_count(n)
            cuts = [0, W // 3, W // 2, W]
            shards, prof = profiled(ctx, lambda: b"".join(ctx.msm_bases_windows_dev(h, sc, n, cuts[i], cuts[i + 1]) for i in range(3)))
            assert ctx.g1_sum(shards) == want, (c, mix, "window ranges")
            assert MARK not in prof, sorted(prof)
            # and the table call on the same handle, after them
            assert ctx.msm_bases_run_dev(h, sc, n) == want, (c, mix)


@pytest.mark.parametrize("c", CS)
def test_the_table_is_the_path_taken(co, ctxs, c):
    """no silent fall-back: an eligible call shows the marker, exactly one accumulation and one reduced bucket set; the same call on a context created
    under BZK_MSM_BASES_TABLE=0 shows no marker and its set holds no table"""
    n = 4097
    scb = scalars("uniform", n, c)
    sc = to_dev(scb)
    torch.cuda.synchronize()
    want = want_of(co, n, scb, ("uniform", 0))
    on, off = ctxs(c), ctxs(0)
    with Loaded(co, on, n) as h:
        got, prof = profiled(on, lambda: on.msm_bases_run_dev(h, sc, n))
        assert got == want
        assert MARK in prof and prof["msm_accumulate"][0] == 1, prof
        assert "msm_bitsum" in prof and prof["msm_bitsum"][0] == 1, prof  # one bucket set reduced, whatever the window count
    with Loaded(co, off, n) as h:
        assert off.msm_bases_table_info(h) == {"c": 0, "levels": 0, "table_bytes": 0}
        got, prof = profiled(off, lambda: off.msm_bases_run_dev(h, sc, n))
        assert got == want
        assert MARK not in prof, sorted(prof)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", CS)
def test_partition_and_sort_fronts_over_the_same_table(co, ctxs, c, n):
    """one handle, two contexts: the shared form of the partition front (bins without a window, 64-bit intermediate pairs) and the pair sort"""
    part, sort = ctxs(c, "partition"), ctxs(c, "sort")
    with Loaded(co, part, n) as h:
        for mix in MIXES:
            scb = scalars(mix, n, c)
            sc = to_dev(scb)
            torch.cuda.synchronize()
            want = want_of(co, n, scb, (mix, c if mix == "carry" else 0))
            assert part.msm_bases_run_dev(h, sc, n) == want, ("partition", c, n, mix)
            assert sort.msm_bases_run_dev(h, sc, n) == want, ("sort", c, n, mix)
        if n == SIZES[-1]:  # a prefix: the table's stride stays the set's
            m = n - 1000
            scb = scalars("half-equal", m, c)
            sc = to_dev(scb)
            torch.cuda.synchronize()
            want = want_of(co, m, scb, ("half-equal", 0))
            assert part.msm_bases_run_dev(h, sc, m) == want, ("partition, prefix", c)
            assert sort.msm_bases_run_dev(h, sc, m) == want, ("sort, prefix", c)


@pytest.mark.parametrize("c", CS)
def test_the_front_of_the_table_call_is_the_one_asked_for(co, ctxs, c):
    """no silent fall-back: the partition context's table call holds msm_digits and the three passes behind it and no pair sort; the sort context's holds the
    pair sort and none of the passes; both show the table marker and one accumulation"""
    n = 4097
    part, sort = ctxs(c, "partition"), ctxs(c, "sort")
    scb = scalars("uniform", n, c)
    sc = to_dev(scb)
    torch.cuda.synchronize()
    want = want_of(co, n, scb, ("uniform", 0))
    with Loaded(co, part, n) as h:
        got, p = profiled(part, lambda: part.msm_bases_run_dev(h, sc, n))
        assert got == want
        got, s = profiled(sort, lambda: sort.msm_bases_run_dev(h, sc, n))
        assert got == want
    assert {MARK, "msm_digits", "msm_front_scan", "msm_front_scatter", "msm_front_bins"} <= set(p) and "msm_sort_pairs" not in p and "msm_offsets" not in p, sorted(p)
    assert {MARK, "msm_digits", "msm_sort_pairs", "msm_offsets"} <= set(s) and not any(k.startswith("msm_front") for k in s), sorted(s)
    assert p["msm_accumulate"][0] == 1 and s["msm_accumulate"][0] == 1


def test_a_context_with_a_forced_window_or_split_keeps_the_pipeline(co):
    """a context created with BZK_MSM_C or a BZK_MSM_SPLIT* setting beside BZK_MSM_BASES_TABLE=1 may load a table but never runs from it"""
    n = 4097
    scb = scalars("uniform", n, 16)
    sc = to_dev(scb)
    torch.cuda.synchronize()
    want = want_of(co, n, scb, ("uniform", 0))
    for extra in ({"BZK_MSM_C": "12"}, {"BZK_MSM_SPLIT": "2", "BZK_MSM_SPLIT_MIN_LOG": "12"}):
        ctx = _ctx_with_env({"BZK_MSM_BASES_TABLE": "1", "BZK_MSM_BASES_TABLE_C": "16", **extra})
        try:
            with Loaded(co, ctx, n) as h:
                got, prof = profiled(ctx, lambda: ctx.msm_bases_run_dev(h, sc, n))
                assert got == want, extra
                assert MARK not in prof, (extra, sorted(prof))
        finally:
            ctx.close()


@pytest.mark.parametrize("n", [1, 4097])
@pytest.mark.parametrize("c", CS)
def test_the_handle_reports_its_table(co, ctxs, c, n):
    """112 bytes x levels x n, levels = the windows of the signed c-bit recoding; device_bytes grows by exactly that over the same set without a table"""
    on, off = ctxs(c), ctxs(0)
    with Loaded(co, on, n) as h, Loaded(co, off, n) as h0:
        t = on.msm_bases_table_info(h)
        levels = (256 + c - 1) // c
        assert t == {"c": c, "levels": levels, "table_bytes": 112 * levels * n}
        i, i0 = on.msm_bases_info(h), off.msm_bases_info(h0)
        assert i["n"] == i0["n"] == n and i["forms"] == i0["forms"]
        assert i["device_bytes"] == i0["device_bytes"] + t["table_bytes"]
        assert i0["device_bytes"] == 112 * n * i0["forms"]


def test_by_default_a_small_set_and_a_g2_set_carry_no_table(co, ctxs):
    """the default rule builds a table for 2^19 < n <= 2^20 G1 points only; G2 sets never own one, whatever the knob says"""
    n = 4097
    ctx = ctxs(None)
    with Loaded(co, ctx, n) as h:
        assert ctx.msm_bases_table_info(h)["table_bytes"] == 0
        assert ctx.msm_bases_info(h)["device_bytes"] == 112 * n * ctx.msm_bases_info(h)["forms"]
    on = ctxs(16)
    m = 63
    d2 = to_dev(co.g2_bases(4343, 0, m, nthreads=co.ncpu()))
    torch.cuda.synchronize()
    h2 = on.msm_bases_load_dev(d2, m, g2=True)
    try:
        assert on.msm_bases_table_info(h2) == {"c": 0, "levels": 0, "table_bytes": 0}
    finally:
        on.msm_bases_free(h2)


def test_a_parameter_set_loads_its_queries_without_tables(co):
    """the prover's MSMs are throughput-flagged or de-duplicated and never run from a set's table: after a device set-up and a proof under
    BZK_MSM_BASES_TABLE=1 the CRS holds resident query sets and none of them owns a table"""
    import array
    r1 = synth_r1cs(30, seed=4242 + 30)
    csr = []
    for which in range(3):
        rp, col, val = array.array("I", [0]), array.array("I"), []
        for row in r1["rows"]:
            for v, cf in row[which]:
                col.append(v)
                val.append(pr.fr_to_mont_bytes(cf))
            rp.append(len(col))
        csr.append((len(r1["rows"]), rp.tobytes(), col.tobytes(), b"".join(val)))
    ctx = _ctx_with_env({"BZK_MSM_BASES_TABLE": "1", "BZK_MSM_BASES_TABLE_C": "11"})
    try:
        ph, _vk = ctx.groth16_setup(csr, r1["n_in"], r1["n_aux"], fr_bytes(fr_list(5, 99)))
        A, B, Cm = r1cs_to_csr(co, r1)
        zb = fr_bytes(r1["z"])
        az, bz, cz = co.r1cs_eval(A, B, Cm, zb, nthreads=co.ncpu())
        r, s = fr_bytes(fr_list(2, 8))[:32], fr_bytes(fr_list(2, 8))[32:]
        assert len(ctx.groth16_prove(ph, zb, az, bz, cz, r, s)) == 387
        info = ctx.params_resident_info(ph)
        assert info["sets"] >= 1 and info["device_bytes"] > 0, info
        assert info["table_bytes"] == 0, info
        ctx.params_free(ph)
    finally:
        ctx.close()
