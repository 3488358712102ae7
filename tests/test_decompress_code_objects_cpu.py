"""Resources of the key-decompression kernel (eddsa.hip jubjub_decompress_kernel), read from the gfx950 code object the build left
(tools/kernel_resources.py, as tests/test_eddsa_code_objects_cpu.py does): it exists exactly once, with no scratch, no spills, no LDS, and few enough
registers for at least two waves per SIMD (256 VGPRs at most; DESIGN.md records the count) - the dependent squaring chain has nothing else to hide
its latency behind."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "witfill.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")


def test_decompress_kernel_exists_once_without_scratch_or_spills():
    rows = [r for r in kr.resources() if r["kernel"] == "jubjub_decompress_kernel"]
    assert len(rows) == 1 and rows[0]["object"] == "eddsa", [(r["object"], r["kernel"]) for r in kr.resources() if r["object"] == "eddsa"]
    r = rows[0]
    assert r["scratch"] == 0 and r["spill"] == 0 and r["lds"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 256, r


def test_the_transaction_kernels_beside_it_have_no_scratch_either():
    rows = {r["kernel"]: r for r in kr.resources() if r["object"] == "eddsa"}
    for k in ("mpn_tx_tuple_kernel", "mpn_tx_verdict_kernel"):
        assert rows[k]["scratch"] == 0 and rows[k]["spill"] == 0, rows[k]
