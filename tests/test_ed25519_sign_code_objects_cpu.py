"""Resources of the Ed25519 signer's kernels (ed_sign.hip: ed25519_sign_kernel, ed25519_keys_kernel, l1_tx_sign_kernel, l1_tx_sign_hash_kernel), read
from the gfx950 code object the build left (tools/kernel_resources.py: resource metadata only, as tests/test_sign_code_objects_cpu.py does).  Each
exists exactly once, in a code object of its own; no kernel has a private segment or a spilled register; registers, LDS and private segment
equal the figures of the table in DESIGN.md 3.17, so the document cannot drift."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "ed_sign.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")

KERNELS = ("ed25519_sign_kernel", "ed25519_keys_kernel", "l1_tx_sign_kernel", "l1_tx_sign_hash_kernel")


def _documented():
    """{kernel: (vector registers, accumulation registers, LDS bytes, private segment bytes)} from the table rows of DESIGN.md 3.17"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.17"):]
    out = {}
    for m in re.finditer(r"^\| (\d+) \| (\d+) \| (\d+) \| (\d+) \| `(\w+_kernel)` \|", sec, re.M):  # the name last: section 3.16's reader takes name-first rows
        out[m.group(5)] = tuple(int(m.group(k)) for k in range(1, 5))
    return out


def test_kernels_in_their_own_code_object():
    rows = [r for r in kr.resources() if r["object"] == "ed_sign"]
    assert sorted(r["kernel"] for r in rows) == sorted(KERNELS), [r["kernel"] for r in rows]
    assert [r["kernel"] for r in kr.resources() if r["kernel"] in KERNELS and r["object"] != "ed_sign"] == []
    for r in rows:
        assert r["wg"] % 64 == 0, r
        if r["kernel"] in KERNELS[:3]:
            assert r["wg"] == 64 and r["lds"] == 0, r   # one wave per block, nothing shared: a lane never waits for another


def test_no_private_segment_and_no_spill():
    for r in kr.resources():
        if r["object"] == "ed_sign":
            assert r["scratch"] == 0 and r["spill"] == 0, r


def test_resources_are_the_documented_ones():
    doc = _documented()
    assert sorted(doc) == sorted(KERNELS), doc
    for r in kr.resources():
        if r["object"] == "ed_sign":
            assert (r["vgpr"], r["agpr"], r["lds"], r["scratch"]) == doc[r["kernel"]], (r, doc[r["kernel"]])
