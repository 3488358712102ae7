"""bzk_g1_subgroup_check_batch / bzk_g2_subgroup_check_batch and their _dev forms on the GPU (bazuka_amd/csrc/subgroup.hip: sg_g1_kernel, sg_g2_kernel,
one lane per point) against [r] P == identity from the oracle and, byte for byte, against the ctx = NULL route, on the case table of
tests/subgroup_cases.py: points of every prime order of the cofactors share wavefronts with subgroup points, malformed records and flagged identities."""
import pytest

from bazuka_amd import lib as L
import subgroup_cases as S

pytestmark = pytest.mark.gpu
GROUPS = ("g1", "g2")
ROUND = 1 << 18   # subgroup.hip SG_ROUND


def _pick(group, n, shift=0):
    recs, inf, want, kinds = S.table(group)
    sz, m = S.SIZE[group], len(inf)
    idx = [(i + shift) % m for i in range(n)]
    return b"".join(recs[sz * i:sz * i + sz] for i in idx), bytes(inf[i] for i in idx), bytes(want[i] for i in idx)


@pytest.mark.parametrize("group", GROUPS)
def test_case_table_through_both_entries(bzk, group):
    import torch
    from util import to_dev
    recs, inf, want, kinds = S.table(group)
    n = len(inf)
    got = bzk.subgroup_check_batch(group, recs, inf)
    assert got == want, [(i, k, g, w) for i, (k, g, w) in enumerate(zip(kinds, got, want)) if g != w]
    assert got == L.host_subgroup_check_batch(group, recs, inf)
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    dp, di = to_dev(recs), to_dev(inf)
    torch.cuda.synchronize()
    bzk.subgroup_check_batch_dev(group, dp, di, n, ok)
    assert bytes(ok.cpu().numpy().tobytes()) == want
    # no flags: the flagged records are read as points
    bare = L.host_subgroup_check_batch(group, recs, None)
    assert bzk.subgroup_check_batch(group, recs, None) == bare and bare != want
    ok.fill_(7)
    bzk.subgroup_check_batch_dev(group, dp, None, n, ok)
    assert bytes(ok.cpu().numpy().tobytes()) == bare


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes(bzk, group, n):
    import torch
    from util import to_dev
    recs, inf, want = _pick(group, n, shift=n)
    assert bzk.subgroup_check_batch(group, recs, inf) == want
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    dp, di = to_dev(recs), to_dev(inf)
    torch.cuda.synchronize()
    bzk.subgroup_check_batch_dev(group, dp, di, n, ok)
    assert bytes(ok.cpu().numpy().tobytes()) == want


@pytest.mark.parametrize("group", GROUPS)
def test_one_call_just_above_the_round_size(bzk, group):
    """the case table tiled past a round boundary: identical bytes on either side of it get identical verdicts"""
    import torch
    from util import to_dev
    recs, inf, want, kinds = S.table(group)
    m = len(inf)
    n = ROUND + m + 1
    reps = n // m + 1
    sz = S.SIZE[group]
    trecs, tinf, twant = (recs * reps)[:sz * n], (inf * reps)[:n], (want * reps)[:n]
    assert bzk.subgroup_check_batch(group, trecs, tinf) == twant
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    dp, di = to_dev(trecs), to_dev(tinf)
    torch.cuda.synchronize()
    bzk.subgroup_check_batch_dev(group, dp, di, n, ok)
    assert bytes(ok.cpu().numpy().tobytes()) == twant


def test_arguments(bzk):
    lib = L.load_library()
    recs, inf, want, kinds = S.table("g1")
    ok = L.C.create_string_buffer(b"\x07" * 2, 2)
    assert lib.bzk_g1_subgroup_check_batch(bzk.h, None, None, 0, None) == 0
    assert lib.bzk_g1_subgroup_check_batch(bzk.h, None, None, 2, ok) == -1 and ok.raw == b"\x07" * 2
    assert lib.bzk_g2_subgroup_check_batch(bzk.h, recs, None, 2, None) == -1
    assert lib.bzk_g1_subgroup_check_batch_dev(bzk.h, None, None, 0, None) == 0
    assert lib.bzk_g1_subgroup_check_batch_dev(bzk.h, None, None, 2, None) == -1


def test_checked_loader_proves_the_same_bytes_and_names_a_bad_point(bzk):
    from util import fr_bytes, fr_list
    blob, parts, r1, params, (zb, az, bz, cz) = S.small_key()
    shape = (r1["n_in"], r1["n_aux"], params["a_density"], params["b_density"])
    ph, vkb = bzk.params_load_bellman(blob, *shape)
    ph2, vkb2 = bzk.params_load_bellman_checked(blob, *shape)
    assert vkb2 == vkb and ph2.value
    r, s = fr_bytes(fr_list(2, 8))[:32], fr_bytes(fr_list(2, 8))[32:]
    p1 = bzk.groth16_prove(ph, zb, az, bz, cz, r, s)
    assert bzk.groth16_prove(ph2, zb, az, bz, cz, r, s) == p1
    bzk.params_free(ph2)
    lib = L.load_library()
    for array, index in (("b_g2", len(parts["b_g2"]) // 192 - 1), ("h", 3), ("vk", 2)):
        bad = S.tampered_key(array, index)
        with pytest.raises(L.ParamsCheckError, match=r"%s\[%d\].*outside the order-r subgroup" % ("the verifying key" if array == "vk" else array, index)) as e:
            bzk.params_load_bellman_checked(bad, *shape)
        assert e.value.report == (S.ARRAYS.index(array), index, 0, 0)
        h = L.C.c_void_p(5)
        report = (L.C.c_uint64 * 4)()
        st = lib.bzk_params_load_bellman_checked(bzk.h, bad, len(bad), shape[0], shape[1], shape[2], shape[3], L.C.byref(h), None, 0, report)
        assert st == -1 and not h.value and tuple(report) == (S.ARRAYS.index(array), index, 0, 0)   # no handle
        ph3, _ = bzk.params_load_bellman(bad, *shape)   # the unchecked loader still takes it: the new check is what refuses
        bzk.params_free(ph3)
    assert bzk.groth16_prove(ph, zb, az, bz, cz, r, s) == p1   # the context is healthy after the refusals
    bzk.params_free(ph)


def test_params_check_on_the_device_equals_the_host_route(bzk):
    blob, parts, *_ = S.small_key()
    blobs = [blob] + [S.tampered_key(a, 1) for a in S.ARRAYS] + [blob[:-5]]
    for b in blobs:
        assert bzk.bellman_params_check(b) == L.host_bellman_params_check(b)
    assert bzk.bellman_params_check(blob) == (1, (0, 0, 0, 0))
    assert bzk.bellman_params_check(blobs[7]) == (0, (6, 1, 0, 0))
