#!/usr/bin/env python3
"""Measures batched Groth16 verification: bzk_groth16_verify_batch on the device against the same call without a context (the per-proof functions
over the host field on the host's threads - what bzk_groth16_verify costs on 16 threads; the parent has nothing else).  Needs an MI355X: no
fallback.

  sizes      proofs/s at n = 64 .. 2^16 proofs of one five-input key (the rows of tests/verify_cases.py taken cyclically: verifying, refused and
             dead-pair lanes mixed), host clock, copies and the key's preparation included; device and host run alternately, three runs each,
             and the ranges are kept.  Every device result is compared with the host's.
  kernels    milliseconds of the three kernels at each size (event pairs around the launches, in a run of their own).
  crossing   the smallest measured n from which the device stops losing.

usage: python tools/verify_batch_bench.py [--out profiles/groth16_verify_batch.json] [--max-log 16]"""
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

SIZES = (64, 256, 1024, 4096, 1 << 14, 1 << 16)


def spread(v):
    return {"runs_s": v, "min_s": min(v), "max_s": max(v), "median_s": sorted(v)[len(v) // 2]}


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groth16_verify_batch.json"))
    ap.add_argument("--max-log", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "verify_batch_bench needs a GPU"
    torch.cuda.set_device(0)
    import verify_cases as V
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    vkb, n_inputs, rows, single = V.table(1)
    assert n_inputs == 5
    res = {"device": torch.cuda.get_device_name(0), "host_threads": L.load_library().bzk_host_default_threads(), "n_inputs": n_inputs,
           "verifying_share": sum(single) / len(single), "sizes": []}
    for n in SIZES:
        if n > 1 << a.max_log:
            continue
        inputs, proofs, want, _ = V.batch(1, n, 5)
        assert ctx.groth16_verify_batch(vkb, inputs, n_inputs, proofs) == want   # also the warm-up (workspace, code object)
        dev, host = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            got = ctx.groth16_verify_batch(vkb, inputs, n_inputs, proofs)
            t1 = time.perf_counter()
            ref = L.host_groth16_verify_batch(vkb, inputs, n_inputs, proofs)
            t2 = time.perf_counter()
            assert got == want and ref == want
            dev.append(t1 - t0)
            host.append(t2 - t1)
        ctx.prof_enable(True)
        ctx.prof_reset()
        ctx.groth16_verify_batch(vkb, inputs, n_inputs, proofs)
        kernels = {k: ms for k, (cnt, ms) in ctx.prof_dump().items() if k.startswith("g16v_")}
        ctx.prof_enable(False)
        row = {"n": n, "device": dict(spread(dev), per_s=n / med(dev)), "host_threads": dict(spread(host), per_s=n / med(host)),
               "ratio": med(host) / med(dev), "ratio_range": [min(host) / max(dev), max(host) / min(dev)], "kernels_ms": kernels}
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    wins = [r["n"] for r in res["sizes"] if r["ratio"] >= 1]
    res["device_stops_losing_at_n"] = min(wins) if wins else None
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
