"""bzk_g1_subgroup_check_batch / bzk_g2_subgroup_check_batch without a device (ctx = NULL: the per-point functions of bazuka_amd/csrc/bzk_subgroup.cuh
over the host field, on host threads) and the same functions in their DEVICE-field instantiation, run on the CPU by the stand-alone program
tests/host/_subgroup_check (built by build() with the bound assertions of bzk_fp28.cuh and the host sanitizers on), against [r] P == identity from the
oracle on the case table of tests/subgroup_cases.py: subgroup points, random curve points, a point of every prime order of the cofactors (alone and
added to a subgroup point), malformed records and flagged identities."""
import os
import subprocess
import sys

import pytest

from bazuka_amd import lib as L
import subgroup_cases as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GROUPS = ("g1", "g2")


def _mismatches(got, want, kinds):
    return [(i, k, g, w) for i, (k, g, w) in enumerate(zip(kinds, got, want)) if g != w]


@pytest.mark.parametrize("group", GROUPS)
def test_host_threads_equal_the_oracle_on_the_case_table(group):
    recs, inf, want, kinds = S.table(group)
    assert {0, 1, 2} == set(want) and kinds.count("torsion") >= 12
    got = L.host_subgroup_check_batch(group, recs, inf)
    assert got == want, _mismatches(got, want, kinds)
    # without the flags the flagged records are read as points: zeros are off the curve, 0xff bytes are out of range, the third is outside the subgroup
    sz = S.SIZE[group]
    bare = bytes(S.oracle_verdict(group, recs[sz * i:sz * i + sz]) for i in range(len(inf)))
    assert L.host_subgroup_check_batch(group, recs, None) == bare and bare != want


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sizes(group, n):
    recs, inf, want, kinds = S.table(group)
    sz, m = S.SIZE[group], len(inf)
    idx = [(7 * i + n) % m for i in range(n)]
    got = L.host_subgroup_check_batch(group, b"".join(recs[sz * i:sz * i + sz] for i in idx), bytes(inf[i] for i in idx))
    assert got == bytes(want[i] for i in idx)


def test_one_host_thread():
    """BZK_HOST_THREADS is read once per process: a child"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from bazuka_amd import lib as L\nimport subgroup_cases as S\n"
            "for g in ('g1', 'g2'):\n"
            "    recs, inf, want, kinds = S.table(g)\n"
            "    assert L.host_subgroup_check_batch(g, recs, inf) == want\n"
            "print('one thread ok')\n") % (ROOT, HERE)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, BZK_HOST_THREADS="1"))
    assert p.returncode == 0 and "one thread ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


@pytest.mark.parametrize("group", GROUPS)
def test_device_field_instantiation_on_the_cpu(group, tmp_path):
    exe = os.path.join(HERE, "host", "_subgroup_check")
    assert os.path.exists(exe), "tests/host/_subgroup_check not built (build() compiles it)"
    recs, want = S.finite(group)
    f = tmp_path / (group + ".bin")
    f.write_bytes(recs)
    p = subprocess.run([exe, group, str(f)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert p.stdout.split() == ["verdicts", "".join(str(v) for v in want)]


def test_arguments():
    lib = L.load_library()
    E_ARG = -1
    for group, fn, fn_dev in (("g1", lib.bzk_g1_subgroup_check_batch, lib.bzk_g1_subgroup_check_batch_dev),
                              ("g2", lib.bzk_g2_subgroup_check_batch, lib.bzk_g2_subgroup_check_batch_dev)):
        recs, inf, want, kinds = S.table(group)
        assert fn(None, None, None, 0, None) == 0                                  # n = 0
        assert L.host_subgroup_check_batch(group, b"") == b""
        ok = L.C.create_string_buffer(b"\x07" * 2, 2)
        assert fn(None, None, None, 2, ok) == E_ARG and fn(None, recs, None, 2, None) == E_ARG
        assert ok.raw == b"\x07" * 2                                               # nothing written
        assert fn_dev(None, recs, None, 2, ok) == E_ARG and ok.raw == b"\x07" * 2  # the device form needs a context
        assert fn(None, recs, None, 2, ok) == 0 and ok.raw == want[:2]             # inf may be NULL
