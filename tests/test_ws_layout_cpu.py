"""The arithmetic of bzk::WsLayout (bazuka_amd/csrc/bzk_ws.h), which lays every device call's temporaries out in the context's workspace slab,
run on the CPU through a harness of its own (tests/host/_ws_check.so includes the very header).  What a call declares is what it reserves: offsets are
256-byte aligned and disjoint, the reserved size is the end of the last buffer, a slab one byte short is refused before anything is bound, and a
size that overflows is refused instead of wrapping."""
import ctypes as C
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BUFS = 64


@pytest.fixture(scope="module")
def hc():
    so = os.path.join(ROOT, "tests", "host", "_ws_check.so")
    if not os.path.exists(so):
        pytest.skip("tests/host/_ws_check.so not built (build() compiles it)")
    h = C.CDLL(so)
    h.ws_check_layout.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint64)]
    h.ws_check_layout.restype = C.c_int
    return h


def layout(hc, bufs, slab=None):
    """bufs: [(element size, count)].  -> (status, offsets, bytes, bound offsets); slab None: a slab of exactly bytes()"""
    n = len(bufs)
    arr = C.c_uint64 * max(n, 1)
    elem, count = arr(*[b[0] for b in bufs]), arr(*[b[1] for b in bufs])
    off, bound, total = arr(), arr(), C.c_uint64(0)
    if slab is None:
        st = hc.ws_check_layout(elem, count, n, 2 ** 64 - 1, off, C.byref(total), bound)
        if st != 0:
            return st, None, None, None
        slab = total.value
    st = hc.ws_check_layout(elem, count, n, slab, off, C.byref(total), bound)
    return st, list(off[:n]), total.value, list(bound[:n])


def random_bufs(rnd):
    sizes = [1, 2, 4, 8, 16, 32, 48, 96, 144, 192, 288, 384]
    counts = [0, 0, 1, 2, 255, 256, 257, 4096, 65537, rnd.randrange(1, 2 ** 20), rnd.randrange(1, 2 ** 31)]
    return [(rnd.choice(sizes), rnd.choice(counts)) for _ in range(rnd.randrange(0, MAX_BUFS + 1))]


def test_offsets_are_aligned_and_disjoint_and_bytes_is_the_end_of_the_last_buffer(hc):
    rnd = random.Random(7)
    cases = [random_bufs(rnd) for _ in range(300)] + [[], [(4, 0)], [(32, 0), (1, 0)], [(1, 1)], [(1, 256), (1, 1)], [(1, 257), (0, 5), (4, 3)]]
    for bufs in cases:
        st, off, total, bound = layout(hc, bufs)
        assert st == 0, bufs
        assert bound == off, bufs  # the variables are pointed at the very offsets the size was computed from
        end = 0
        for (size, count), o in zip(bufs, off):
            assert o % 256 == 0 and o >= end, (bufs, off)  # aligned, and not before the end of any earlier buffer
            assert o - end < 256, (bufs, off)               # and no further than the alignment asks
            end = o + size * count
        assert total == end, (bufs, off, total)
    assert layout(hc, [])[2] == 0 and layout(hc, [(8, 0), (32, 0)])[2] == 0  # nothing taken, or only empty buffers: nothing to reserve


def test_a_slab_one_byte_short_is_refused(hc):
    rnd = random.Random(8)
    for _ in range(200):
        bufs = random_bufs(rnd)
        st, off, total, _ = layout(hc, bufs)
        assert st == 0
        if total == 0:
            continue
        assert layout(hc, bufs, total)[0] == 0
        assert layout(hc, bufs, total + 1)[0] == 0
        assert layout(hc, bufs, total - 1)[0] == 1, bufs  # 1: refused with no variable bound (the hook answers -1 if one was)
        assert layout(hc, bufs, 0)[0] == 1, bufs
    # a trailing empty buffer past the slab's end is refused as well: its address would lie outside
    assert layout(hc, [(1, 1), (4, 0)], 255)[0] == 1 and layout(hc, [(1, 1), (4, 0)], 256)[0] == 0


def test_a_size_that_overflows_is_refused(hc):
    big = 2 ** 64 - 1
    assert layout(hc, [(32, 2 ** 59)])[0] == 2           # count * size = 2^64
    assert layout(hc, [(32, 2 ** 59 - 1)])[0] == 0       # the largest that fits
    assert layout(hc, [(8, big)])[0] == 2
    assert layout(hc, [(1, big)])[0] == 0
    assert layout(hc, [(1, 1), (1, big - 255)])[0] == 2  # offset 256 + size passes 2^64
    assert layout(hc, [(1, 1), (1, big - 256)])[0] == 0
    assert layout(hc, [(1, big), (1, 0)])[0] == 2        # aligning the next offset wraps
    assert layout(hc, [(4, 2 ** 62), (4, 2 ** 62)])[0] == 2
    assert layout(hc, [(4, 1)] * MAX_BUFS)[0] == 0
    assert layout(hc, [(4, 1)] * (MAX_BUFS + 1))[0] == 2  # more buffers than a layout holds
