"""Resources of the ContractUpdate kernels (bazuka_amd/csrc/updates.hip), read from the gfx950 code object the build left
(tools/kernel_resources.py, as tests/test_l1_code_objects_cpu.py does): registers, LDS and private segment of each equal the table of DESIGN.md
3.12, each exists exactly once, and none has a private segment (no scratch).  Resource figures only."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "updates.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")
KERNELS = ("upd_deposit_sig_kernel", "upd_deposit_leaf_kernel", "upd_withdraw_leaf_kernel", "upd_tree_level_kernel", "upd_inputs_kernel",
           "upd_verdict_kernel")


def design_table():
    """{kernel: (registers, LDS bytes, private segment bytes)} from the table of DESIGN.md 3.12"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 3.12"):]
    section = section[:section.index("\n## ")]
    return {m.group(1): tuple(int(m.group(k).replace(" ", "")) for k in (2, 3, 4))
            for m in re.finditer(r"^\| `(upd_\w+)` \| ([\d ]+) \| ([\d ]+) \| ([\d ]+) \|$", section, re.M)}


def built():
    return {r["kernel"]: r for r in kr.resources() if r["object"] == "updates"}


def test_every_kernel_once_and_no_others():
    rows = [r["kernel"] for r in kr.resources() if r["object"] == "updates"]
    assert sorted(rows) == sorted(KERNELS), rows
    assert sorted(design_table()) == sorted(KERNELS)


@pytest.mark.parametrize("kernel", KERNELS)
def test_resources_equal_the_design_table(kernel):
    r = built()[kernel]
    assert (r["vgpr"], r["lds"], r["scratch"]) == design_table()[kernel], r  # vgpr: the unified count, as in the table of 3.11


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    assert built()[kernel]["scratch"] == 0, built()[kernel]


def test_signature_kernel_keeps_the_verifiers_footprint():
    r = built()["upd_deposit_sig_kernel"]
    assert r["lds"] == 708 * 64 and r["vgpr"] + r["agpr"] <= 288 and r["spill"] == 0, r  # ed25519_verify_kernel's 272 + 16 and its LDS columns
