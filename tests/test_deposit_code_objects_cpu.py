"""Resources of the deposit-admission kernels (eddsa.hip sha512_kernel, ed25519_verify_kernel, mpn_deposit_verdict_kernel), read from the gfx950
code object the build left (tools/kernel_resources.py, as tests/test_withdraw_code_objects_cpu.py does).  Each exists exactly once; none uses
scratch or spills.  The register bounds are the counts measured when the kernels were written: 92 for SHA-512, 272 + 16 for
the verifier, which holds one signature's hash, reduction and group equation without a split."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "witfill.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")


def _one(kernel):
    rows = [r for r in kr.resources() if r["kernel"] == kernel]
    assert len(rows) == 1 and rows[0]["object"] == "eddsa", [(r["object"], r["kernel"]) for r in kr.resources() if r["object"] == "eddsa"]
    assert rows[0]["scratch"] == 0 and rows[0]["spill"] == 0, rows[0]
    return rows[0]


def test_sha512_kernel_keeps_state_and_schedule_in_registers():
    r = _one("sha512_kernel")
    assert r["lds"] == 0, r
    assert 48 <= r["vgpr"] + r["agpr"] <= 92, r  # 16 + 32 registers of state and ring; measured 92: five waves per SIMD


def test_verify_kernel_is_one_kernel_without_scratch():
    r = _one("ed25519_verify_kernel")
    assert r["lds"] == 708 * 64, r  # 4 x 40 table words, 9 + 8 scalar words per lane: three blocks per CU
    assert 2 * r["lds"] <= 160 * 1024
    assert r["vgpr"] + r["agpr"] <= 288, r  # measured 272 + 16
    assert not [x for x in kr.resources() if x["kernel"] == "ed25519_hram_kernel"]  # no split was needed


def test_verdict_kernel():
    r = _one("mpn_deposit_verdict_kernel")
    assert r["lds"] == 0 and r["vgpr"] + r["agpr"] <= 8, r  # measured 6
