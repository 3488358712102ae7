"""Resources of the point-scaling kernel (rekey.hip: g1_scale_kernel), read from the gfx950 code object the build left (tools/kernel_resources.py, as
tests/test_subgroup_code_objects_cpu.py does).  It exists exactly once, in a code object of its own; no private segment, no spilled register, no
LDS; registers, LDS and private segment equal the figures of the table in DESIGN.md 3.20, so the document cannot drift."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ), reason="bazuka_amd/csrc/_obj not built (build() compiles it)")

KERNELS = ("g1_scale_kernel",)


def _documented():
    """{kernel: (registers, LDS bytes, private segment bytes)} from the rows `| rekey | `kernel` | registers | LDS | private |` of DESIGN.md 3.20 (the unit first:
    section 3.16's reader takes every name-first row from there to the end of the document)"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.20"):]
    out = {}
    for m in re.finditer(r"^\| rekey \| `(g1_scale_\w+)` \| (\d+) \| (\d+) \| (\d+) \|", sec, re.M):
        out[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    return out


def _rows():
    return [r for r in kr.resources() if r["object"] == "rekey"]


def test_one_kernel_in_its_own_code_object():
    rows = _rows()
    assert sorted(r["kernel"] for r in rows) == sorted(KERNELS), [r["kernel"] for r in rows]
    assert [r["kernel"] for r in kr.resources() if r["kernel"].startswith("g1_scale_") and r["object"] != "rekey"] == []
    for r in rows:
        assert r["wg"] == 64, r   # one wave per block: a lane never waits for another


def test_no_private_segment_no_spills_no_lds():
    for r in _rows():
        assert r["scratch"] == 0 and r["lds"] == 0, r
        assert r["spill"] == 0, r


def test_resources_are_the_documented_ones():
    doc = _documented()
    assert sorted(doc) == sorted(KERNELS), doc
    for r in _rows():
        assert (r["vgpr"], r["lds"], r["scratch"]) == doc[r["kernel"]], (r, doc[r["kernel"]])
