"""bzk_groth16_verify_batch_keys / bzk_groth16_verify_groups_dev on the GPU (bazuka_amd/csrc/verify_keys.hip: g16k_prepare_kernel, g16k_miller_kernel,
g16k_finalexp_kernel - the lanes of several keys side by side, every group padded to whole blocks of 64, rounds of 2^16 lanes) against what the
single call says about each row under its key (tests/verify_keys_cases.py over tests/verify_cases.py), element-wise.  Group counts sit around
the block of 64, where the layout can go wrong; every failure names the first differing row by group, index and row name."""
import pytest

import verify_keys_cases as K

pytestmark = pytest.mark.gpu


def _host_form(bzk, groups, seed=None):
    """the groups through key_of: in group order, or (seed) shuffled"""
    if seed is None:
        keys, counts, inputs, proofs, want, where = K.grouped(groups)
        key_of = [k for k, c in enumerate(counts) for _ in range(c)]
    else:
        keys, key_of, inputs, proofs, want, where = K.interleaved(groups, seed)
    got = bzk.groth16_verify_batch_keys(keys, key_of, inputs, proofs)
    assert got == want, K.first_difference(got, want, where)


def _dev_form(bzk, groups):
    import torch
    from util import to_dev
    keys, counts, inputs, proofs, want, where = K.grouped(groups)
    din = to_dev(inputs) if inputs else torch.zeros(1, dtype=torch.uint8, device="cuda")
    dpr = to_dev(proofs)
    ok = torch.full((len(want),), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bzk.groth16_verify_groups_dev(keys, counts, din, dpr, ok)
    got = bytes(ok.cpu().numpy().tobytes())
    assert got == want, K.first_difference(got, want, where)


@pytest.mark.parametrize("counts", [(1, 63), (63, 1), (64, 65), (65, 64)])
def test_two_keys_around_the_block(bzk, counts):
    groups = [K.table_group(0, counts[0], 20 + counts[0]), K.table_group(1, counts[1], 40 + counts[1])]
    _host_form(bzk, groups)
    _dev_form(bzk, groups)


def test_three_keys_of_different_input_counts(bzk):
    groups = [K.table_group(0, 65, 1), K.table_group(1, 1, 2), K.no_input_group(0, 130)]   # n_inputs 2, 5, 0
    assert [g[1] for g in groups] == [2, 5, 0]
    _dev_form(bzk, groups)
    _host_form(bzk, groups)
    _host_form(bzk, groups, seed=5)


@pytest.mark.parametrize("at", [0, 1, 2])
def test_an_empty_group(bzk, at):
    groups = [K.table_group(0, 65, 3), K.table_group(1, 3, 4)]
    groups.insert(at, K.table_group(at % 2, 0, 0))
    assert len(groups[at][4]) == 0
    _dev_form(bzk, groups)
    _host_form(bzk, groups)


def test_an_invalid_key_between_two_valid_groups(bzk):
    groups = [K.table_group(0, 65, 6), K.invalid_group(66, 7), K.table_group(1, 17, 8)]
    assert any(groups[0][4]) and any(groups[2][4]) and groups[1][4] == bytes(66)
    _dev_form(bzk, groups)
    _host_form(bzk, groups, seed=9)


def test_the_wide_key_inside_a_mixed_call(bzk):
    groups = [K.table_group(0, 65, 10), K.wide_group(6), K.table_group(1, 64, 11)]
    assert groups[1][1] == 18 and groups[1][4] == bytes([1, 0, 1, 1, 0, 1])
    _dev_form(bzk, groups)
    _host_form(bzk, groups, seed=12)


def test_device_form_equals_host_form_and_back_to_back_calls(bzk):
    """two calls on one context with different group shapes: the second must not see the first's block table, records or flags"""
    first = [K.table_group(0, 130, 13), K.table_group(1, 65, 14)]
    second = [K.table_group(1, 3, 15), K.no_input_group(1, 64), K.table_group(0, 70, 16)]
    for groups in (first, second, first):
        _dev_form(bzk, groups)
        _host_form(bzk, groups)


def test_round_crossing_with_a_straddling_group(bzk):
    """group 0 fills round 1 up to its last block; group 1 (300 rows) has that block's 64 lanes in round 1 and the other 236 in round 2 on the
    same slab.  A cutter that drops or doubles the straddling group's lanes shows in group 1's verdicts."""
    groups = [K.table_group(0, (1 << 16) - 100, 17), K.table_group(1, 300, 18)]
    keys, counts, inputs, proofs, want, where = K.grouped(groups)
    key_of = [0] * counts[0] + [1] * counts[1]
    got = bzk.groth16_verify_batch_keys(keys, key_of, inputs, proofs)
    assert got[-300:] == want[-300:], K.first_difference(got[-300:], want[-300:], where[-300:])
    assert got == want, K.first_difference(got, want, where)
    _dev_form(bzk, groups)
