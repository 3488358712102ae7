"""Resources of the subgroup-check kernels (subgroup.hip: sg_g1_kernel, sg_g2_kernel), read from the gfx950 code object the build left
(tools/kernel_resources.py, as tests/test_verify_code_objects_cpu.py does).  Each exists exactly once, in a code object of its own; no scratch, no
spilled register; registers, LDS and private segment equal the figures of the table in DESIGN.md 3.13, so the document cannot drift."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ), reason="bazuka_amd/csrc/_obj not built (build() compiles it)")

KERNELS = ("sg_g1_kernel", "sg_g2_kernel")


def _documented():
    """{kernel: (registers, LDS bytes, private segment bytes)} from the rows `| `kernel` | registers | LDS | private |` of DESIGN.md 3.13"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.13"):]
    out = {}
    for m in re.finditer(r"^\| `(sg_\w+)` \| (\d+) \| (\d+) \| (\d+) \|", sec, re.M):
        out[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    return out


def _rows():
    return [r for r in kr.resources() if r["object"] == "subgroup"]


def test_two_kernels_in_their_own_code_object():
    rows = _rows()
    assert sorted(r["kernel"] for r in rows) == sorted(KERNELS), [r["kernel"] for r in rows]
    assert [r["kernel"] for r in kr.resources() if r["kernel"].startswith("sg_") and r["object"] != "subgroup"] == []
    for r in rows:
        assert r["wg"] == 64, r   # one wave per block: a lane never waits for another


def test_no_scratch_and_no_spills():
    for r in _rows():
        assert r["scratch"] == 0 and r["lds"] == 0, r
        assert r["spill"] == 0, r


def test_resources_are_the_documented_ones():
    doc = _documented()
    assert sorted(doc) == sorted(KERNELS), doc
    for r in _rows():
        assert (r["vgpr"], r["lds"], r["scratch"]) == doc[r["kernel"]], (r, doc[r["kernel"]])
