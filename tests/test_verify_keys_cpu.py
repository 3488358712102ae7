"""bzk_groth16_verify_batch_keys without a device (ctx = NULL: bazuka_amd/csrc/verify_keys.hip runs bzk_pairing28.cuh's per-proof functions over the
host field, all proofs of all keys in one task loop) against what the existing single-key call says about each proof under its key, element-wise;
the argument refusals; n = 0.  The groups come from tests/verify_keys_cases.py (rows of tests/verify_cases.py)."""
from bazuka_amd import lib as L
import verify_cases as V
import verify_keys_cases as K

E_ARG = -1


def _per_key(groups):
    """the oracle: the existing single-key batched call, group by group"""
    return [L.host_groth16_verify_batch(g[0], g[2], g[1], g[3]) for g in groups]


def test_interleaved_keys_equal_the_per_key_results():
    groups = [K.table_group(0, 17, 1), K.table_group(1, 17, 2), K.no_input_group(0, 5), K.invalid_group(9, 3), K.no_input_group(1, 5)]
    for g, got in zip(groups, _per_key(groups)):
        assert got == g[4], g[5][0]   # the single-key batched call says what the single call says
    assert any(groups[0][4]) and any(groups[1][4]) and any(groups[2][4]) and not any(groups[3][4])
    for seed in (1, 2):
        keys, key_of, inputs, proofs, want, where = K.interleaved(groups, seed)
        got = L.host_groth16_verify_batch_keys(keys, key_of, inputs, proofs)
        assert got == want, K.first_difference(got, want, where)
    # and in group order (key_of ascending)
    keys, counts, inputs, proofs, want, where = K.grouped(groups)
    key_of = [k for k, c in enumerate(counts) for _ in range(c)]
    got = L.host_groth16_verify_batch_keys(keys, key_of, inputs, proofs)
    assert got == want, K.first_difference(got, want, where)


def test_the_same_key_as_two_key_indices():
    a, b = K.table_group(1, 11, 5), K.table_group(1, 7, 6)
    assert a[0] == b[0]
    keys, key_of, inputs, proofs, want, where = K.interleaved([a, K.table_group(0, 3, 7), b], 4)
    got = L.host_groth16_verify_batch_keys(keys, key_of, inputs, proofs)
    assert got == want, K.first_difference(got, want, where)
    # a key nobody names is not looked at beyond its length
    keys2 = keys + [(bytes(878), 3)]
    assert L.host_groth16_verify_batch_keys(keys2, key_of, inputs, proofs) == want


def test_eighteen_inputs_beside_the_others():
    groups = [K.table_group(0, 4, 8), K.wide_group(3), K.table_group(1, 4, 9)]
    keys, key_of, inputs, proofs, want, where = K.interleaved(groups, 6)
    got = L.host_groth16_verify_batch_keys(keys, key_of, inputs, proofs)
    assert got == want, K.first_difference(got, want, where)


def _raw(keys, key_of, inputs, proofs, n, ok, ctx=None, n_keys=None, vk_off=None):
    vks, off, n_inputs = L._pack_keys(keys)
    if vk_off is not None:
        off = (L.C.c_uint64 * len(vk_off))(*vk_off)
    ko = (L.C.c_uint32 * max(len(key_of), 1))(*key_of)
    return L.load_library().bzk_groth16_verify_batch_keys(ctx, len(keys) if n_keys is None else n_keys, vks, off, n_inputs, ko, inputs, proofs, n, ok)


def test_arguments():
    groups = [K.table_group(0, 2, 1), K.table_group(1, 2, 2)]
    keys, key_of, inputs, proofs, want, _ = K.interleaved(groups, 1)
    n = len(want)
    ok = L.C.create_string_buffer(b"\x07" * n, n)
    assert _raw(keys, key_of, inputs, proofs, n, ok) == 0 and ok.raw == want          # the well-formed call, through the same helper
    ok = L.C.create_string_buffer(b"\x07" * n, n)
    lens = [len(k[0]) for k in keys]
    assert _raw(keys, [0, 2, 1, 0], inputs, proofs, n, ok) == E_ARG                   # key_of[i] >= n_keys
    assert _raw(keys, key_of, inputs, proofs, n, ok, vk_off=[lens[0], 0, lens[0] + lens[1]]) == E_ARG   # vk_off not ascending
    assert _raw(keys, key_of, inputs, proofs, n, ok, vk_off=[0, 877, 877 + lens[1]]) == E_ARG            # a key shorter than 878 bytes
    assert _raw(keys, key_of, inputs, proofs, n, ok, vk_off=[0, lens[0], lens[0] + 877]) == E_ARG
    assert _raw(keys, key_of, inputs, proofs, n, ok, n_keys=0) == E_ARG               # no key, n > 0
    assert _raw(keys, key_of, None, proofs, n, ok) == E_ARG                           # null pointers
    assert _raw(keys, key_of, inputs, None, n, ok) == E_ARG
    assert _raw(keys, key_of, inputs, proofs, n, None) == E_ARG
    lib = L.load_library()
    vks, off, n_inputs = L._pack_keys(keys)
    ko = (L.C.c_uint32 * n)(*key_of)
    assert lib.bzk_groth16_verify_batch_keys(None, 2, None, off, n_inputs, ko, inputs, proofs, n, ok) == E_ARG
    assert lib.bzk_groth16_verify_batch_keys(None, 2, vks, None, n_inputs, ko, inputs, proofs, n, ok) == E_ARG
    assert lib.bzk_groth16_verify_batch_keys(None, 2, vks, off, None, ko, inputs, proofs, n, ok) == E_ARG
    assert lib.bzk_groth16_verify_batch_keys(None, 2, vks, off, n_inputs, None, inputs, proofs, n, ok) == E_ARG
    assert ok.raw == b"\x07" * n                                                      # nothing written by a refused call
    # the device form needs a context
    cnt = (L.C.c_uint64 * 2)(2, 2)
    assert lib.bzk_groth16_verify_groups_dev(None, 2, vks, off, n_inputs, cnt, inputs, proofs, ok) == E_ARG
    assert ok.raw == b"\x07" * n


def test_no_proofs():
    lib = L.load_library()
    assert lib.bzk_groth16_verify_batch_keys(None, 0, None, None, None, None, None, None, 0, None) == 0
    vkb, n_inputs, _, _ = V.table(0)
    assert L.host_groth16_verify_batch_keys([(vkb, n_inputs)], [], b"", b"") == b""
    assert L.host_groth16_verify_batch_keys([], [], b"", b"") == b""
