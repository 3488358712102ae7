#!/usr/bin/env python3
"""Measures a chain of m deltas on the device-resident state: ONE bzk_state_update_chain call (all deltas through the tree together, one launch per
(level, arity), every root compared with its claim) against m bzk_state_update calls on a second handle, one after another - the parent's code
path and the baseline.  Needs an MI355X: no fallback.

  workload   MpnConfig::state_model at L = 15, T = 3 over 4 096 populated accounts; a delta writes 512 of them x (tx_nonce, one balance) = 1 024
             pairs (bench.py's state_device_incremental shape); m = 1, 16, 64, 256.  The claims of the chain are the states the baseline gave.
  clock      host clock around the C calls: planning, uploads, launches, the roots' way back and the commit included; the ctypes arrays are built
             before the clock starts, for both forms alike.  The two forms run alternately in one process, three runs each on fresh deltas,
             ranges kept.  Every state of the chain is compared with the baseline's.
  kernels    milliseconds per launch label of each form (event pairs around the launches, in a run of their own).

usage: python tools/state_chain_bench.py [--out profiles/state_update_chain.json] [--max-m 256]"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bazuka_amd import lib as L  # noqa: E402

MS = (1, 16, 64, 256)
LOG_L, LOG_T, ACCOUNTS, PER_DELTA = 15, 3, 4096, 512


def spread(v):
    return {"runs_s": v, "min_s": min(v), "max_s": max(v), "median_s": sorted(v)[len(v) // 2]}


def med(v):
    return sorted(v)[len(v) // 2]


def limbs(rnd):
    return rnd.randrange(1, 1 << 60).to_bytes(32, "little")  # Montgomery limbs of some non-zero residue: any 32 bytes below r are


class Chain:
    """m deltas as the C arrays both forms read: delta j is pairs d_off[j] .. d_off[j + 1] of loc_off / loc / values"""

    def __init__(self, rnd, accts, m, height0):
        self.m, flat = m, []
        for _ in range(m):
            for a in rnd.sample(accts, PER_DELTA):
                flat.append(((a, 0), limbs(rnd)))
                flat.append(((a, 4, 0, 1), limbs(rnd)))
        per = 2 * PER_DELTA
        self.pairs = len(flat)
        self.d_off = (C.c_uint64 * (m + 1))(*[per * j for j in range(m + 1)])
        off, loc = [0], []
        for l, _ in flat:
            loc.extend(l)
            off.append(len(loc))
        self.loc_off, self.loc = (C.c_uint64 * len(off))(*off), (C.c_uint64 * len(loc))(*loc)
        self.values = C.create_string_buffer(b"".join(v for _, v in flat), 32 * len(flat))
        self.heights = (C.c_uint64 * m)(*range(height0 + 1, height0 + 1 + m))
        self.per = per

    def sequential(self, lib, ctx, h):
        """-> (seconds, the m states)"""
        out, size = C.create_string_buffer(40 * self.m), C.c_uint64()
        lo = C.addressof(self.loc_off)
        t0 = time.perf_counter()
        for j in range(self.m):
            st = lib.bzk_state_update(h, C.c_void_p(lo + 8 * self.per * j), self.loc, C.c_void_p(C.addressof(self.values) + 32 * self.per * j), self.per,
                                      self.heights[j], C.c_void_p(C.addressof(out) + 40 * j), C.byref(size), None)
            assert st == 0, lib.bzk_last_error(ctx.h)
            C.memmove(C.addressof(out) + 40 * j + 32, C.byref(size), 8)
        return time.perf_counter() - t0, out.raw

    def chain(self, lib, ctx, h, claims):
        out, verdict, applied = C.create_string_buffer(40 * self.m), C.create_string_buffer(self.m), C.c_uint64()
        t0 = time.perf_counter()
        st = lib.bzk_state_update_chain(h, self.m, self.d_off, self.loc_off, self.loc, self.values, self.heights, claims, 0, out, verdict, C.byref(applied), None)
        dt = time.perf_counter() - t0
        assert st == 0 and applied.value == self.m and verdict.raw == bytes(self.m), (st, applied.value, lib.bzk_last_error(ctx.h))
        return dt, out.raw


def kernels_of(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    out = {k: {"launches": cnt, "ms": ms} for k, (cnt, ms) in ctx.prof_dump().items()}
    ctx.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_update_chain.json"))
    ap.add_argument("--max-m", type=int, default=256)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "state_chain_bench needs a GPU"
    torch.cuda.set_device(0)
    import pystate as ps
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    lib = ctx.lib
    rnd = random.Random(2024)
    model = ps.model_bincode(ps.mpn_model(LOG_L, LOG_T))
    accts = rnd.sample(range(4 ** LOG_L), ACCOUNTS)
    load = []
    for acc in accts:
        load += [((acc, j), limbs(rnd)) for j in range(4)] + [((acc, 4, 0, 0), limbs(rnd)), ((acc, 4, 0, 1), limbs(rnd))]
    one, many = L.DeviceState(ctx, model), L.DeviceState(ctx, model)  # one: the chain call; many: one bzk_state_update per delta
    assert one.update(load, 1) == many.update(load, 1)
    height = 1
    res = {"device": torch.cuda.get_device_name(0), "model": "MpnConfig::state_model L = 15, T = 3", "accounts": ACCOUNTS, "pairs_per_delta": 2 * PER_DELTA,
           "sizes": []}
    for m in MS:
        if m > a.max_m:
            continue
        new, old = [], []
        for run in range(4):  # run 0 warms both forms up (workspace growth, code objects) and is not kept
            ch = Chain(rnd, accts, m, height)
            height += m
            t_old, want = ch.sequential(lib, ctx, many.h)
            t_new, got = ch.chain(lib, ctx, one.h, want)
            assert got == want and one.root() == many.root()
            if run:
                new.append(t_new)
                old.append(t_old)
        prof = Chain(rnd, accts, m, height)
        height += m
        k_old = kernels_of(ctx, lambda: prof.sequential(lib, ctx, many.h))
        k_new = kernels_of(ctx, lambda: prof.chain(lib, ctx, one.h, None))
        assert one.root() == many.root()
        dev_new = sum(v["ms"] for v in k_new.values()) / 1e3
        row = {"m": m, "pairs": m * 2 * PER_DELTA, "chain": dict(spread(new), per_delta_ms=1e3 * med(new) / m),
               "sequential": dict(spread(old), per_delta_ms=1e3 * med(old) / m), "ratio": med(old) / med(new),
               "ratio_range": [min(old) / max(new), max(old) / min(new)],
               "chain_kernel_s": dev_new, "chain_host_share": max(0.0, 1 - dev_new / med(new)),
               "kernels_chain": k_new, "kernels_sequential": k_old}
        res["sizes"].append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.startswith("kernels_")}), flush=True)
    assert one.stats()["keys"] == many.stats()["keys"]
    one.close()
    many.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
