"""Resources of the L1 transaction kernels (eddsa.hip l1_tx_verify_kernel, l1_tx_hash_kernel, sha3_merkle_level_kernel), read from the gfx950
code object the build left (tools/kernel_resources.py, as tests/test_deposit_code_objects_cpu.py does).  Each exists exactly once; none uses
scratch or spills.  The register bounds are the counts measured when the kernels were written: the verifier keeps
ed25519_verify_kernel's 272 + 16 - the gathered message's twelve words live during the hash only, which is not where the ladder's peak is; the
hash kernel measured 118 (sha3_256_kernel's 108 and the piece list), the level kernel 69 (one permutation over a 64-byte input)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "witfill.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")


def _one(kernel):
    rows = [r for r in kr.resources() if r["kernel"] == kernel]
    assert len(rows) == 1 and rows[0]["object"] == "eddsa", [(r["object"], r["kernel"]) for r in kr.resources() if r["object"] == "eddsa"]
    assert rows[0]["scratch"] == 0 and rows[0]["spill"] == 0, rows[0]
    return rows[0]


def test_verify_kernel_keeps_the_verifiers_footprint():
    r = _one("l1_tx_verify_kernel")
    assert r["lds"] == 708 * 64, r  # the same per-lane LDS columns as ed25519_verify_kernel: three blocks per CU
    assert r["vgpr"] + r["agpr"] <= 288, r  # measured 272 + 16, as ed25519_verify_kernel: one wave per SIMD at least (512 registers)


def test_hash_kernel_keeps_state_and_pieces_in_registers():
    r = _one("l1_tx_hash_kernel")
    assert r["lds"] == 0, r  # the piece list indexed by a variable would show here (or as scratch)
    assert 50 <= r["vgpr"] + r["agpr"] <= 120, r  # fifty registers of state; measured 118: four waves per SIMD


def test_level_kernel():
    r = _one("sha3_merkle_level_kernel")
    assert r["lds"] == 0, r
    assert 50 <= r["vgpr"] + r["agpr"] <= 72, r  # measured 69: seven waves per SIMD


def test_helper_kernels():
    for name, bound in (("sha3_merkle_place_kernel", 24), ("sha3_merkle_roots_kernel", 16)):  # measured 20 and 13
        r = _one(name)
        assert r["lds"] == 0 and r["vgpr"] + r["agpr"] <= bound, r
