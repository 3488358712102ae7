"""Resources of the witness-only evaluation's kernels (r1cs_eval.hip: r1cs_eval_kernel, r1cs_sat_kernel), read from the gfx950 code object the build left
(tools/kernel_resources.py, as tests/test_withdraw_sign_code_objects_cpu.py does).  They exist exactly once, in a code object of their own; they have no
private segment and spill nothing - eighteen 64-bit columns, two nine-limb operands and a running sum stay in registers, nothing is indexed at run time;
registers, LDS and private segment equal the figures of the table in DESIGN.md 3.19, so the document cannot drift.  Only resource figures are looked at."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "r1cs_eval.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")

KERNELS = ("r1cs_eval_kernel", "r1cs_sat_kernel")


def _documented():
    """{kernel: (vector registers, accumulation registers, LDS bytes, private segment bytes)} from the table rows of DESIGN.md 3.19 whose first column
    is `r1cs`"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.19"):]
    out = {}
    for m in re.finditer(r"^\| r1cs \| `(\w+_kernel)` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|", sec, re.M):
        out[m.group(1)] = tuple(int(m.group(k)) for k in range(2, 6))
    return out


def test_kernels_in_their_own_code_object_without_a_private_segment():
    rows = [r for r in kr.resources() if r["object"] == "r1cs_eval"]
    assert sorted(r["kernel"] for r in rows) == sorted(KERNELS), [r["kernel"] for r in rows]
    assert sorted(r["object"] for r in kr.resources() if r["kernel"] in KERNELS) == ["r1cs_eval"] * 2
    for r in rows:
        assert r["wg"] == 256 and r["lds"] == 0, r   # the wave's partial sums travel through registers
        assert r["scratch"] == 0 and r["spill"] == 0, r
        assert r["waves"] >= 4, r                    # a gather-bound kernel: several waves per SIMD to hide the reads


def test_resources_are_the_documented_ones():
    doc = _documented()
    assert sorted(doc) == sorted(KERNELS), doc
    for r in kr.resources():
        if r["object"] == "r1cs_eval":
            assert (r["vgpr"], r["agpr"], r["lds"], r["scratch"]) == doc[r["kernel"]], (r, doc[r["kernel"]])
