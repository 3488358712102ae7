"""Resources of the per-point multiplication kernels (pmul.hip), read from the gfx950 code object the build left (tools/kernel_resources.py, as
tests/test_rekey_code_objects_cpu.py does).  The five kernels exist exactly once, in a code object of their own, one wavefront per block; no LDS and no
private segment anywhere; no spilled register on G1 and in the preparation kernels, and on G2 the count DESIGN.md 3.21 states; registers, LDS and
private segment equal the figures of the table in DESIGN.md 3.21, so the document cannot drift.  Resources only: the assembly is not read."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ), reason="bazuka_amd/csrc/_obj not built (build() compiles it)")

KERNELS = ("pmul_range_kernel", "pmul_prep_kernel", "pmul_prep_powers_kernel", "g1_pmul_kernel", "g2_pmul_kernel")


def _documented():
    """{kernel: (registers, LDS bytes, private segment bytes)} from the rows `| pmul | `kernel` | registers | LDS | private |` of DESIGN.md 3.21, and the
    spill count the section states for g2_pmul_kernel"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.21"):]
    out = {}
    for m in re.finditer(r"^\| pmul \| `(\w+_kernel)` \| (\d+) \| (\d+) \| (\d+) \|", sec, re.M):
        out[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    spills = re.search(r"`g2_pmul_kernel` spills (\d+) registers", sec)
    return out, int(spills.group(1)) if spills else 0


def _rows():
    return [r for r in kr.resources() if r["object"] == "pmul"]


def test_the_kernels_in_their_own_code_object():
    rows = _rows()
    assert sorted(r["kernel"] for r in rows) == sorted(KERNELS), [r["kernel"] for r in rows]
    assert [r["kernel"] for r in kr.resources() if (r["kernel"] in KERNELS or "pmul" in r["kernel"]) and r["object"] != "pmul"] == []
    for r in rows:
        assert r["wg"] == 64, r   # one wave per block: a lane never waits for another, and g2_pmul_kernel finds its record by its lane index


def test_no_private_segment_no_lds_and_the_stated_spills():
    _, g2_spills = _documented()
    for r in _rows():
        assert r["scratch"] == 0 and r["lds"] == 0, r
        assert r["spill"] == (g2_spills if r["kernel"] == "g2_pmul_kernel" else 0), r


def test_resources_are_the_documented_ones():
    doc, _ = _documented()
    assert sorted(doc) == sorted(KERNELS), doc
    for r in _rows():
        assert (r["vgpr"], r["lds"], r["scratch"]) == doc[r["kernel"]], (r, doc[r["kernel"]])
