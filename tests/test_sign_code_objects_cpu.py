"""Resources of the signer's kernels (sign.hip: jubjub_sign_kernel, jubjub_keys_kernel and the transaction signer's two glue kernels), read from the
gfx950 code object the build left (tools/kernel_resources.py, as tests/test_verify_code_objects_cpu.py does).  Each exists exactly once, in a code
object of its own; registers, LDS and private segment equal the figures of the table in DESIGN.md 3.16, so the document cannot drift."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "sign.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")

KERNELS = ("jubjub_sign_kernel", "jubjub_keys_kernel", "mpn_tx_sign_inputs_kernel", "mpn_tx_sign_hash_kernel")


def _documented():
    """{kernel: (vector registers, accumulation registers, LDS bytes, private segment bytes)} from the table rows of DESIGN.md 3.16"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.16"):]
    out = {}
    for m in re.finditer(r"^\| `(\w+_kernel)` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|", sec, re.M):
        out[m.group(1)] = tuple(int(m.group(k)) for k in range(2, 6))
    return out


def test_kernels_in_their_own_code_object():
    rows = [r for r in kr.resources() if r["object"] == "sign"]
    assert sorted(r["kernel"] for r in rows) == sorted(KERNELS), [r["kernel"] for r in rows]
    assert [r["kernel"] for r in kr.resources() if r["kernel"] in KERNELS and r["object"] != "sign"] == []
    for r in rows:
        assert r["wg"] % 64 == 0, r
        if r["kernel"] in KERNELS[:2]:
            assert r["wg"] == 64 and r["lds"] == 0, r   # one wave per block, nothing shared: a lane never waits for another


def test_resources_are_the_documented_ones():
    doc = _documented()
    assert sorted(doc) == sorted(KERNELS), doc
    for r in kr.resources():
        if r["object"] == "sign":
            assert (r["vgpr"], r["agpr"], r["lds"], r["scratch"]) == doc[r["kernel"]], (r, doc[r["kernel"]])
