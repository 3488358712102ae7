"""bzk_bellman_params_check without a device (ctx = NULL: bellman's `Parameters::read(.., checked = true)` as a verdict, the whole check on host threads)
on the small key of tests/subgroup_cases.py: 1 for the intact key; for each of the seven arrays, one point replaced by a curve point outside the
subgroup gives 0 with the report naming exactly that array and index, while the same blob still passes bzk_bellman_params_decode - the new check is
what refuses it."""
import pytest

from bazuka_amd import lib as L
import subgroup_cases as S


def test_intact_key_passes():
    blob = S.small_key()[0]
    assert L.host_bellman_params_check(blob) == (1, (0, 0, 0, 0))
    assert L.host_bellman_params_check(blob + b"tail") == (1, (0, 0, 0, 0))   # trailing bytes are the caller's business, as in decode


@pytest.mark.parametrize("array", S.ARRAYS)
def test_one_point_outside_the_subgroup_is_named(array):
    blob, parts, *_ = S.small_key()
    count = 6 if array == "vk" else len(parts[array]) // {"ic": 97, "b_g2": 192}.get(array, 96)
    assert count >= 2
    for index in sorted({0, count // 2, count - 1}):
        bad = S.tampered_key(array, index)
        assert L.host_bellman_params_check(bad) == (0, (S.ARRAYS.index(array), index, 0, 0)), (array, index)
        L.bellman_params_decode(bad)   # does not raise: the point is canonical and on its curve


def test_first_failure_in_file_order_and_decode_failures():
    blob, parts, *_ = S.small_key()
    # two bad points: the one earlier in the file is reported
    p = dict(parts)
    p["a"] = S.outside_point("g1") + p["a"][96:]
    p["l"] = p["l"][:96] + S.outside_point("g1") + p["l"][192:]
    both = L.bellman_params_encode(*[p[k] for k in S.ARRAYS])
    assert L.host_bellman_params_check(both) == (0, (3, 1, 0, 0))
    # what decode refuses is refused here with code 2 and its place: an off-curve h point, a truncated blob
    off_h = 3 * 96 + 3 * 192 + 4 + 96 * (len(parts["ic"]) // 97) + 4
    broken = bytearray(blob)
    broken[off_h + 96 * 2 + 95] ^= 1
    with pytest.raises(L.BzkError):
        L.bellman_params_decode(bytes(broken))
    assert L.host_bellman_params_check(bytes(broken)) == (0, (2, 2, 2, 0))
    assert L.host_bellman_params_check(blob[:-5]) == (0, (7, 0, 2, 0))


def test_arguments():
    lib = L.load_library()
    blob = S.small_key()[0]
    report = (L.C.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.bzk_bellman_params_check(None, None, 0, report) == -1 and list(report) == [9, 9, 9, 9]
    assert lib.bzk_bellman_params_check(None, blob, len(blob), None) == -1
    out = L.C.c_void_p()
    assert lib.bzk_params_load_bellman_checked(None, blob, len(blob), 4, 1, b"\1" * 5, b"\1" * 5, L.C.byref(out), None, 0, report) == -1   # needs a context
