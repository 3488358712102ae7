"""Resources of the chain's kernels (state.hip state_chain_hash_kernel<T>, state_chain_hash_coop_kernel<T>, T = 2 .. 8), read from the gfx950 code
objects the build left (tools/kernel_resources.py, as tests/test_l1_code_objects_cpu.py does).  The yardstick is not a fixed count but the kernel of
the same width that bzk_state_update launches today, in the same build: poseidon29_kernel<T> for the lane-per-node form, poseidon29_coop_kernel<T>
(poseidon29_coop5_kernel for T = 5) for the cooperative one.  Fetching the inputs through source indices must cost no scratch, no spill and no
occupancy step over hashing them from a dense array.

Measured when the kernels were written (registers: chain kernel / its yardstick, waves per SIMD):
    T   lane-per-node          cooperative
    2    83 /  83  (5)         105 / 105  (4)
    3   114 / 114  (4)         123 / 123  (4)      poseidon29_kernel<3> keeps 32 B of scratch, the chain kernel none
    4   139 / 138  (3)         141 / 141  (3)
    5   148 / 148  (3)         159 / 159  (3)
    6   216 / 215  (2)         177 / 177  (2)      one spilled register in both lane-per-node kernels
    7   258 / 258  (1)         195 / 195  (2)
    8   251 / 252  (2)         213 / 213  (2)      the yardstick spills one register, the chain kernel none"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.OBJ) or not os.path.exists(os.path.join(kr.OBJ, "state.o")),
                                reason="bazuka_amd/csrc/_obj not built (build() compiles it)")
WIDTHS = range(2, 9)


@pytest.fixture(scope="module")
def rows():
    return kr.resources()


def _one(rows, obj, kernel):
    got = [r for r in rows if r["kernel"] == kernel]
    assert len(got) == 1 and got[0]["object"] == obj, (kernel, [(r["object"], r["kernel"]) for r in got])
    return got[0]


def _held(mine, yard):
    assert mine["scratch"] <= yard["scratch"] and mine["spill"] <= yard["spill"], (mine, yard)
    assert mine["lds"] == 0, mine
    assert mine["waves"] >= yard["waves"], (mine, yard)  # the registers do not reach the next occupancy step above the yardstick's


@pytest.mark.parametrize("t", WIDTHS)
def test_lane_per_node_kernel_keeps_the_hash_kernels_footprint(rows, t):
    _held(_one(rows, "state", "state_chain_hash_kernel<%d>" % t), _one(rows, "poseidon", "poseidon29_kernel<%d>" % t))


@pytest.mark.parametrize("t", WIDTHS)
def test_cooperative_kernel_keeps_the_cooperative_hash_kernels_footprint(rows, t):
    yard = "poseidon29_coop5_kernel" if t == 5 else "poseidon29_coop_kernel<%d>" % t
    _held(_one(rows, "state", "state_chain_hash_coop_kernel<%d>" % t), _one(rows, "poseidon", yard))


def test_index_kernels_are_small(rows):
    for name in ("state_chain_gather_kernel", "state_chain_commit_kernel"):
        r = _one(rows, "state", name)
        assert r["scratch"] == 0 and r["spill"] == 0 and r["lds"] == 0 and r["vgpr"] + r["agpr"] <= 24, r  # measured 12
