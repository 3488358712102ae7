"""GPU parity of the MSM's partition front (bazuka_amd/csrc/msm_impl.cuh section 3d, msm_front.cuh): a plain call's signed digits bucketed by a
histogram / scan / scatter / bin pass instead of the radix sort.  Contexts created under BZK_MSM_FRONT=partition and =sort with BZK_MSM_C in
{12, 13, 16} must return the CPU oracle's bytes - and so each other's - on both curves, for sizes around the tile (4096 scalars) and the workgroup
boundaries, for scalar vectors that empty, fill or overflow single bins (every size x mix on G1; on G2 every mix up to 4097 points and two mixes
above), over raw and resident bases, a prefix of a resident set, two and three
window ranges in flight and canonical input; and the launch labels must say that the partition path is the one that ran."""
import os

import pytest
import torch

from oracle import pyref as pr
from util import dev_bytes, fr_bytes, fr_list, rand_scalars_bytes, to_dev

pytestmark = pytest.mark.gpu
R = pr.R_MOD
SIZES = [1, 255, 257, 4095, 4097, (1 << 13) + 1, (1 << 16) + 4321]
MIXES = ["uniform", "zero", "equal", "r-1", "carry", "small", "half-equal"]
CS = [12, 13, 16]


def _ctx_with_env(env):
    """a context of its own created under `env` (the MSM knobs are read when a context is created)"""
    from bazuka_amd import Bzk
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return Bzk(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    """contexts by (window size, front), created on first use, closed with the module"""
    made = {}

    def get(c, front, **extra):
        key = (c, front, tuple(sorted(extra.items())))
        if key not in made:
            made[key] = _ctx_with_env({"BZK_MSM_C": str(c), "BZK_MSM_FRONT": front, **extra})
        return made[key]

    yield get
    for ctx in made.values():
        ctx.close()


def _carry_values(c):
    """scalars whose raw digit is 2^(c-1) resp. 2^(c-1) + 1 in every window: the first stays positive, the second turns negative and carries"""
    out = []
    for d in ((1 << (c - 1)), (1 << (c - 1)) + 1):
        out.append(sum(d << (c * w) for w in range(253 // c)) % R)
    return out


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
        a, b = (pr.fr_to_mont_bytes(v) for v in _carry_values(c))
        return ((a + b) * (n // 2 + 1))[:32 * n]
    if mix == "small":
        rng = pr.SplitMix64(5 + n)
        return fr_bytes([rng.fr() % (1 << 44) for _ in range(n)])
    assert mix == "half-equal"
    return pr.fr_to_mont_bytes(fr_list(1, 78)[0]) * (n // 2) + rand_scalars_bytes(n - n // 2, 2000 + n)


_bases, _want = {}, {}


def bases_of(co, g2, n):
    """host bytes of the first n points of one seeded set per curve (a prefix of a set is a set)"""
    if g2 not in _bases:
        _bases[g2] = (co.g2_bases if g2 else co.g1_bases)(4242, 0, SIZES[-1], nthreads=co.ncpu())
    return _bases[g2][:n * (192 if g2 else 96)]


def want_of(co, g2, n, scb, tag):
    """the oracle's result, computed once per input and shared by every window size and form"""
    key = (g2, n, tag)
    if key not in _want:
        _want[key] = (co.msm_g2 if g2 else co.msm_g1)(bases_of(co, g2, n), scb, nthreads=co.ncpu())
    return _want[key]


def _check(co, ctxs, c, g2, n, mixes):
    part, sort = ctxs(c, "partition"), ctxs(c, "sort")
    db = to_dev(bases_of(co, g2, n))
    run = (lambda ctx, sc: ctx.msm_g2_dev(db, sc, n)) if g2 else (lambda ctx, sc: ctx.msm_g1_dev(db, sc, n))
    for mix in mixes:
        scb = scalars(mix, n, c)
        sc = to_dev(scb)
        torch.cuda.synchronize()
        want = want_of(co, g2, n, scb, (mix, c if mix == "carry" else 0))
        got_p, got_s = run(part, sc), run(sort, sc)
        assert got_p == want, ("partition", c, g2, n, mix)
        assert got_s == want, ("sort", c, g2, n, mix)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", CS)
def test_g1_raw_bases_every_size_and_mix(co, ctxs, c, n):
    _check(co, ctxs, c, False, n, MIXES)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", CS)
def test_g2_raw_bases_every_size(co, ctxs, c, n):
    """G2 runs the same curve-independent chain, so it is not given G1's full product: every mix up to 4097 points, and only the uniform and half-equal
    vectors at the two larger sizes (the G2 oracle is several times slower per point); the other mixes at those sizes run on G1 alone"""
    _check(co, ctxs, c, True, n, MIXES if n <= 4097 else ["uniform", "half-equal"])


@pytest.mark.parametrize("g2", [False, True])
@pytest.mark.parametrize("c", CS)
def test_resident_prefix_and_canonical_forms(co, ctxs, c, g2):
    n = (1 << 13) + 1
    part, sort = ctxs(c, "partition"), ctxs(c, "sort")
    db = to_dev(bases_of(co, g2, n))
    torch.cuda.synchronize()
    hp, hs = part.msm_bases_load_dev(db, n, g2=g2), sort.msm_bases_load_dev(db, n, g2=g2)
    try:
        for mix in ("uniform", "half-equal", "carry"):
            scb = scalars(mix, n, c)
            sc = to_dev(scb)
            torch.cuda.synchronize()
            want = want_of(co, g2, n, scb, (mix, c if mix == "carry" else 0))
            assert part.msm_bases_run_dev(hp, sc, n, g2=g2) == want, ("resident", mix)
            assert sort.msm_bases_run_dev(hs, sc, n, g2=g2) == want, ("resident, sort", mix)
        # a shorter prefix of the resident set
        m = 4097
        scb = scalars("uniform", m, c)
        sc = to_dev(scb)
        torch.cuda.synchronize()
        want = want_of(co, g2, m, scb, ("uniform", 0))
        assert part.msm_bases_run_dev(hp, sc, m, g2=g2) == want
        assert sort.msm_bases_run_dev(hs, sc, m, g2=g2) == want
        # canonical (non-Montgomery) input, values >= r among it: reduced before the recoding on both paths
        can = [R + 5, 2 * R + 1, (1 << 256) - 1, R, 7, 0] + fr_list(m - 6, 31)
        scc = to_dev(b"".join(v.to_bytes(32, "little") for v in can))
        torch.cuda.synchronize()
        want = want_of(co, g2, m, fr_bytes([v % R for v in can]), ("canonical", 0))
        run = (lambda ctx: ctx.msm_g2_dev(db[:192 * m], scc, m, canonical=True)) if g2 else (lambda ctx: ctx.msm_g1_dev(db[:96 * m], scc, m, canonical=True))
        assert run(part) == want
        assert run(sort) == want
        assert part.msm_bases_run_dev(hp, scc, m, g2=g2, canonical=True) == want
    finally:
        part.msm_bases_free(hp)
        sort.msm_bases_free(hs)


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("c", CS)
def test_window_ranges_in_flight(co, ctxs, c, parts):
    """a stand-alone G1 call as two and three window ranges in flight: every range buckets its own windows through the partition passes"""
    n = (1 << 16) + 4321
    split = {"BZK_MSM_SPLIT": str(parts), "BZK_MSM_SPLIT_MIN_LOG": "12"}
    part, sort = ctxs(c, "partition", **split), ctxs(c, "sort", **split)
    db = to_dev(bases_of(co, False, n))
    torch.cuda.synchronize()
    hp, hs = part.msm_bases_load_dev(db, n), sort.msm_bases_load_dev(db, n)
    try:
        for mix in ("uniform", "half-equal"):
            scb = scalars(mix, n, c)
            sc = to_dev(scb)
            torch.cuda.synchronize()
            want = want_of(co, False, n, scb, (mix, 0))
            part.prof_enable(True)
            part.prof_reset()
            assert part.msm_bases_run_dev(hp, sc, n) == want, (parts, mix)
            prof = part.prof_dump()
            part.prof_enable(False)
            assert prof.get("msm_accumulate", (0, 0.0))[0] == parts and prof.get("msm_front_bins", (0, 0.0))[0] == parts, prof
            assert "msm_sort_pairs" not in prof
            assert sort.msm_bases_run_dev(hs, sc, n) == want, (parts, mix, "sort")
            assert part.msm_g1_dev(db, sc, n) == want, (parts, mix, "raw bases")
    finally:
        part.msm_bases_free(hp)
        sort.msm_bases_free(hs)


@pytest.mark.parametrize("c", CS)
def test_the_partition_front_is_the_path_taken(co, ctxs, c):
    """no silent fall-back: the launch labels of a partition-context call hold msm_digits and the three passes behind it and no pair sort; the sort
    context's hold the pair sort and none of the passes"""
    n = 4097
    db = to_dev(bases_of(co, False, n))
    sc = to_dev(scalars("uniform", n, c))
    torch.cuda.synchronize()

    def labels(ctx):
        ctx.prof_enable(True)
        ctx.prof_reset()
        ctx.msm_g1_dev(db, sc, n)
        out = set(ctx.prof_dump())
        ctx.prof_enable(False)
        return out

    p, s = labels(ctxs(c, "partition")), labels(ctxs(c, "sort"))
    assert {"msm_digits", "msm_front_scan", "msm_front_scatter", "msm_front_bins"} <= p and "msm_sort_pairs" not in p and "msm_offsets" not in p, p
    assert {"msm_digits", "msm_sort_pairs", "msm_offsets"} <= s and not any(k.startswith("msm_front") for k in s), s
