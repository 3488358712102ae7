"""Groups of rows for the several-key verifier's tests (tests/test_verify_keys_cpu.py, tests/test_gpu_verify_keys.py), all taken from
tests/verify_cases.py: a group is (key bytes, n_inputs, inputs, proofs, expected verdict bytes, row names), the expected verdicts being what
the SINGLE call bzk_groth16_verify says about each row under the group's key - never what the code under test says."""
import functools
import random

from bazuka_amd import lib as L
import verify_cases as V


def table_group(key_index, count, seed):
    vkb, n_inputs, _, _ = V.table(key_index)
    inputs, proofs, want, names = V.batch(key_index, count, seed)
    return vkb, n_inputs, inputs, proofs, want, ["table(%d): %s" % (key_index, n) for n in names]


def no_input_group(which, count):
    """count rows of V.no_input_keys()[which] (0: the inputs folded into IC_0, 1: IC_0 at infinity), its five proofs taken cyclically"""
    vk0, proofs, single = V.no_input_keys()[which]
    pick = [i % 5 for i in range(count)]
    return (vk0, 0, b"", b"".join(proofs[387 * k:387 * k + 387] for k in pick), bytes(single[k] for k in pick),
            ["no inputs %d: proof %d" % (which, k) for k in pick])


def wide_group(count):
    vkb, n_inputs, inputs, proofs, single = V.wide_key()
    pick = [i % 3 for i in range(count)]
    return (vkb, n_inputs, b"".join(inputs[576 * k:576 * k + 576] for k in pick), b"".join(proofs[387 * k:387 * k + 387] for k in pick),
            bytes(single[k] for k in pick), ["18 inputs: row %d" % k for k in pick])


@functools.lru_cache(maxsize=None)
def invalid_key():
    """table(0)'s key with one byte of gamma.x flipped: off its curve, so the single call refuses every proof under it (asserted here)"""
    vkb, n_inputs, rows, single = V.table(0)
    bad = vkb[:387] + bytes([vkb[387] ^ 1]) + vkb[388:]
    assert single[0] == 1 and L.groth16_verify(bad, rows[0][1], rows[0][2]) is False
    assert L.host_groth16_verify_batch(bad, rows[0][1] + rows[1][1], n_inputs, rows[0][2] + rows[1][2]) == bytes(2)
    return bad


def invalid_group(count, seed):
    """rows that verify under table(0)'s key, given under the invalid one: every verdict 0"""
    _, n_inputs, inputs, proofs, want, names = table_group(0, count, seed)
    assert count < 4 or any(want)
    return invalid_key(), n_inputs, inputs, proofs, bytes(count), ["invalid key: " + n for n in names]


def grouped(groups):
    """the groups as bzk_groth16_verify_groups_dev takes them: (keys [(vk, n_inputs)], counts, inputs, proofs, expected, [(group, index, name)])"""
    return ([(g[0], g[1]) for g in groups], [len(g[4]) for g in groups], b"".join(g[2] for g in groups), b"".join(g[3] for g in groups),
            b"".join(g[4] for g in groups), [(k, i, nm) for k, g in enumerate(groups) for i, nm in enumerate(g[5])])


def interleaved(groups, seed):
    """the same rows in a shuffled order through key_of: (keys, key_of, inputs, proofs, expected, [(group, index, name)])"""
    where = [(k, i) for k, g in enumerate(groups) for i in range(len(g[4]))]
    random.Random(seed).shuffle(where)
    row_in = lambda g, i: g[2][32 * g[1] * i:32 * g[1] * (i + 1)]
    return ([(g[0], g[1]) for g in groups], [k for k, _ in where], b"".join(row_in(groups[k], i) for k, i in where),
            b"".join(groups[k][3][387 * i:387 * i + 387] for k, i in where), bytes(groups[k][4][i] for k, i in where),
            [(k, i, groups[k][5][i]) for k, i in where])


def first_difference(got, want, where):
    """None, or (group, index within the group, row name, got, want) of the first differing row"""
    if len(got) != len(want):
        return ("length", len(got), len(want))
    for g, w, (k, i, name) in zip(got, want, where):
        if g != w:
            return (k, i, name, g, w)
    return None
