"""Resources of the signature verifier's kernel (eddsa.hip jubjub_verify_kernel), read from the gfx950 code object the build left
(tools/kernel_resources.py, as tests/test_defer_sig_code_objects_cpu.py does): it exists exactly once, with no scratch and no spills.  No register cap:
the kernel runs alone, not beside an accumulation wave (DESIGN.md records the count)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "witfill.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")


def test_verify_kernel_has_no_scratch_and_no_spills():
    rows = [r for r in kr.resources() if r["kernel"] == "jubjub_verify_kernel"]
    assert len(rows) == 1 and rows[0]["object"] == "eddsa", [(r["object"], r["kernel"]) for r in kr.resources() if r["object"] == "eddsa"]
    r = rows[0]
    assert r["scratch"] == 0 and r["spill"] == 0, r
    assert r["lds"] == 4 * 27 * 4 * 64, r  # the lanes' tables {1, 2, 3, 4} pk: 108 words each
