"""Resource limits of the signature-ladder kernels of the deferred witness (witfill.hip wf_ladder_kernel / wf_ladder_fill_kernel), read from the
gfx950 code object the build left (tools/kernel_resources.py, as tests/test_code_objects_cpu.py does for the other kernels): no scratch, no spills,
and at most 304 VGPRs (AGPRs included) - the rule of the other fill kernels, so that a wave fits beside an accumulation wave."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "witfill.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")


@pytest.mark.parametrize("kernel", ["wf_ladder_kernel", "wf_ladder_fill_kernel"])
def test_ladder_kernels_fit_beside_the_accumulation(kernel):
    rows = [r for r in kr.resources() if r["object"] == "witfill" and r["kernel"] == kernel]
    assert len(rows) == 1, [r["kernel"] for r in kr.resources() if r["object"] == "witfill"]
    r = rows[0]
    assert r["scratch"] == 0 and r["spill"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 304, r
