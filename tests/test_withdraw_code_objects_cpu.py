"""Resources of the withdrawal-admission kernels (eddsa.hip sha3_256_kernel, mpn_withdraw_inputs_kernel, mpn_withdraw_verdict_kernel), read from
the gfx950 code object the build left (tools/kernel_resources.py, as tests/test_decompress_code_objects_cpu.py does).  The fingerprint kernel - the
SHA3-256 kernel, which the public batch entry shares - exists exactly once; its 25-lane state must be in registers, so no scratch and no spills
(50 registers of state: DESIGN.md records the count), and no LDS."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "witfill.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")


def test_fingerprint_kernel_exists_once_without_scratch_or_spills():
    rows = [r for r in kr.resources() if r["kernel"] == "sha3_256_kernel"]
    assert len(rows) == 1 and rows[0]["object"] == "eddsa", [(r["object"], r["kernel"]) for r in kr.resources() if r["object"] == "eddsa"]
    r = rows[0]
    assert r["scratch"] == 0 and r["spill"] == 0 and r["lds"] == 0, r
    assert 50 <= r["vgpr"] + r["agpr"] <= 128, r  # the state alone is 50; at most 128 keeps four waves per SIMD


def test_the_two_small_kernels_exist_once_without_scratch_or_spills():
    for k in ("mpn_withdraw_inputs_kernel", "mpn_withdraw_verdict_kernel"):
        rows = [r for r in kr.resources() if r["kernel"] == k]
        assert len(rows) == 1 and rows[0]["object"] == "eddsa", k
        assert rows[0]["scratch"] == 0 and rows[0]["spill"] == 0 and rows[0]["lds"] == 0, rows[0]
