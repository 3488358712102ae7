"""Resources of the several-key Groth16 verifier's kernels (verify_keys.hip: g16k_prepare_kernel, g16k_miller_kernel, g16k_finalexp_kernel), read
from the gfx950 code object the build left (tools/kernel_resources.py, as tests/test_verify_code_objects_cpu.py does).  Each exists exactly
once, in a code object of its own; registers, LDS and private segment equal the figures of the table in DESIGN.md 3.14, so the document cannot
drift - and a key that stopped being wave-uniform (held in vector registers) would show here as a larger private segment."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

KERNELS = ("g16k_prepare_kernel", "g16k_miller_kernel", "g16k_finalexp_kernel")


def _documented():
    """{kernel: (registers, LDS bytes, private segment bytes)} from the rows `| `kernel` | registers | LDS | private |` of DESIGN.md 3.14"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 3.14"):]
    out = {}
    for m in re.finditer(r"^\| `(g16k_\w+)` \| (\d+) \| (\d+) \| (\d+) \|", sec, re.M):
        out[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    return out


def test_three_kernels_in_their_own_code_object():
    assert os.path.exists(os.path.join(kr.OBJ, "verify_keys.o")), "bazuka_amd/csrc/_obj/verify_keys.o not built (build() compiles it)"
    rows = [r for r in kr.resources() if r["object"] == "verify_keys"]
    assert sorted(r["kernel"] for r in rows) == sorted(KERNELS), [r["kernel"] for r in rows]
    assert [r["kernel"] for r in kr.resources() if r["kernel"].startswith("g16k_") and r["object"] != "verify_keys"] == []
    for r in rows:
        assert r["wg"] == 64, r   # one wave per block: a block, and so a wavefront, belongs to one key


def test_resources_are_the_documented_ones():
    doc = _documented()
    assert sorted(doc) == sorted(KERNELS), doc
    rows = [r for r in kr.resources() if r["object"] == "verify_keys"]
    assert len(rows) == 3, rows
    for r in rows:
        assert (r["vgpr"], r["lds"], r["scratch"]) == doc[r["kernel"]], (r, doc[r["kernel"]])
