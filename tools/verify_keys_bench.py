#!/usr/bin/env python3
"""Measures Groth16 verification of proofs of several keys: ONE bzk_groth16_verify_batch_keys call (the lanes of all keys side by side, one set of
launches per round) against the existing bzk_groth16_verify_batch called once per key, one call after another - the parent's code path and the
baseline.  Needs an MI355X: no fallback.

  sizes      three keys (the two table keys of tests/verify_cases.py, 2 and 5 inputs, and the five-input production key of
             tests/golden/groth16_production_case.json), n proofs each, n = 64, 1 024, 4 096, 2^14; the rows are given interleaved (proof i
             of key i mod 3), so the new call also pays its grouping.  Host clock, copies and key preparation included; the two forms run
             alternately in one process, three runs each, ranges kept.  Every verdict of the new call is compared with the three calls'.
  kernels    milliseconds of the kernels of each form (event pairs around the launches, in a run of their own).

usage: python tools/verify_keys_bench.py [--out profiles/groth16_verify_keys.json] [--max-log 14]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bazuka_amd import lib as L  # noqa: E402

SIZES = (64, 1024, 4096, 1 << 14)


def spread(v):
    return {"runs_s": v, "min_s": min(v), "max_s": max(v), "median_s": sorted(v)[len(v) // 2]}


def med(v):
    return sorted(v)[len(v) // 2]


def kernels_of(ctx, call, prefix):
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    out = {k: {"launches": cnt, "ms": ms} for k, (cnt, ms) in ctx.prof_dump().items() if k.startswith(prefix)}
    ctx.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_verify_keys.json"))
    ap.add_argument("--max-log", type=int, default=14)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "verify_keys_bench needs a GPU"
    torch.cuda.set_device(0)
    import verify_cases as V
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    pvk, pin, pother, pproof = V.production_fixture()
    res = {"device": torch.cuda.get_device_name(0), "host_threads": L.load_library().bzk_host_default_threads(), "keys": 3, "sizes": []}
    for n in SIZES:
        if n > 1 << a.max_log:
            continue
        groups = []   # (vk, n_inputs, inputs, proofs)
        for key in (0, 1):
            vkb, n_inputs, _, _ = V.table(key)
            inputs, proofs, _, _ = V.batch(key, n, 5 + key)
            groups.append((vkb, n_inputs, inputs, proofs))
        groups.append((pvk, 5, b"".join(pin if i % 2 == 0 else pother for i in range(n)), pproof * n))
        keys = [(g[0], g[1]) for g in groups]
        key_of = (L.C.c_uint32 * (3 * n))(*[i % 3 for i in range(3 * n)])
        row_in = lambda g, i: g[2][32 * g[1] * i:32 * g[1] * (i + 1)]
        inputs = b"".join(row_in(groups[i % 3], i // 3) for i in range(3 * n))
        proofs = b"".join(groups[i % 3][3][387 * (i // 3):387 * (i // 3 + 1)] for i in range(3 * n))

        def three_calls():
            return [ctx.groth16_verify_batch(g[0], g[2], g[1], g[3]) for g in groups]

        def one_call():
            return ctx.groth16_verify_batch_keys(keys, key_of, inputs, proofs)

        want = three_calls()   # also the warm-up (workspace, code objects)
        assert any(want[0]) and not all(want[0]) and want[2] == bytes([1, 0] * (n // 2))
        interleaved = bytes(want[i % 3][i // 3] for i in range(3 * n))
        assert one_call() == interleaved
        new, old = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            got = one_call()
            t1 = time.perf_counter()
            ref = three_calls()
            t2 = time.perf_counter()
            assert got == interleaved and ref == want
            new.append(t1 - t0)
            old.append(t2 - t1)
        row = {"n_per_key": n, "proofs": 3 * n, "one_call": dict(spread(new), per_s=3 * n / med(new)),
               "three_calls": dict(spread(old), per_s=3 * n / med(old)), "ratio": med(old) / med(new),
               "ratio_range": [min(old) / max(new), max(old) / min(new)],
               "kernels_one_call": kernels_of(ctx, one_call, "g16k_"), "kernels_three_calls": kernels_of(ctx, three_calls, "g16v_")}
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
