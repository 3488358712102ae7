"""Resources of the withdrawal producer's kernel (withdraw_sign.hip: mpn_withdraw_sign_kernel), read from the gfx950 code object the build left
(tools/kernel_resources.py, as tests/test_sign_code_objects_cpu.py does).  It exists exactly once, in a code object of its own; it has no private
segment and spills nothing; registers, LDS and private segment equal the figures of the table in DESIGN.md 3.18, so the document cannot drift.
Only resource figures are looked at."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "withdraw_sign.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")

KERNELS = ("mpn_withdraw_sign_kernel",)


def _documented():
    """{kernel: (vector registers, accumulation registers, LDS bytes, private segment bytes)} from the table rows of DESIGN.md 3.18, whose first
    column is text (which keeps them apart from the rows the tests of 3.16 and 3.17 read)"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.18"):]
    out = {}
    for m in re.finditer(r"^\| withdraw \| `(\w+_kernel)` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|", sec, re.M):
        out[m.group(1)] = tuple(int(m.group(k)) for k in range(2, 6))
    return out


def test_kernel_in_its_own_code_object():
    rows = [r for r in kr.resources() if r["object"] == "withdraw_sign"]
    assert sorted(r["kernel"] for r in rows) == sorted(KERNELS), [r["kernel"] for r in rows]
    assert [r["object"] for r in kr.resources() if r["kernel"] in KERNELS] == ["withdraw_sign"]
    for r in rows:
        assert r["wg"] == 64 and r["lds"] == 0, r   # one wave per block, nothing shared: a lane never waits for another
        assert r["scratch"] == 0 and r["spill"] == 0, r
        assert r["vgpr"] + r["agpr"] <= 512, r


def test_resources_are_the_documented_ones():
    doc = _documented()
    assert sorted(doc) == sorted(KERNELS), doc
    for r in kr.resources():
        if r["object"] == "withdraw_sign":
            assert (r["vgpr"], r["agpr"], r["lds"], r["scratch"]) == doc[r["kernel"]], (r, doc[r["kernel"]])
