#!/usr/bin/env python3
"""Measures batched Ed25519 key derivation and signing: bzk_ed25519_keys_batch and bzk_ed25519_sign_batch on the device against the same calls
without a context (the same per-lane functions on the host's threads).  Needs an MI355X: no fallback.

  sizes      rows/s at n = 256 .. 2^16, all rows distinct (a key of its own and a 64-byte message of its own per row), host clock, copies
             included; device and host run alternately, three runs each, and the ranges are kept.  Every device result is compared with the
             host's bytes.
  kernels    milliseconds of ed25519_sign_kernel / ed25519_keys_kernel at each size (event pairs around the launches, in a run of their own).
  verifier   milliseconds of ed25519_verify_kernel over the signatures just made, at the largest size on the same machine: the signer's kernel
             against the verifier's.
  crossing   the smallest measured n from which the device stops losing.

usage: python tools/ed25519_sign_bench.py [--out profiles/ed25519_sign_batch.json] [--max-log 16]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)

import torch  # noqa: E402

from bazuka_amd import lib as L  # noqa: E402

SIZES = (256, 1024, 4096, 1 << 14, 1 << 16)
MSG_LEN = 64


def spread(v):
    return {"runs_s": v, "min_s": min(v), "max_s": max(v), "median_s": sorted(v)[len(v) // 2]}


def med(v):
    return sorted(v)[len(v) // 2]


def alternate(dev_fn, host_fn):
    want = host_fn()
    assert dev_fn() == want  # also the warm-up (workspace, code object, table)
    dev, host = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        got = dev_fn()
        t1 = time.perf_counter()
        ref = host_fn()
        t2 = time.perf_counter()
        assert got == want and ref == want
        dev.append(t1 - t0)
        host.append(t2 - t1)
    return dev, host


def kernel_ms(ctx, fn, label):
    ctx.prof_enable(True)
    ctx.prof_reset()
    fn()
    ms = {k: v for k, (cnt, v) in ctx.prof_dump().items() if k == label}
    ctx.prof_enable(False)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ed25519_sign_batch.json"))
    ap.add_argument("--max-log", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ed25519_sign_bench needs a GPU"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    rnd = random.Random(20261020)
    nmax = max(n for n in SIZES if n <= 1 << a.max_log)
    seeds = [b"ed25519 sign bench %d " % i + bytes(rnd.randrange(256) for _ in range(rnd.randrange(40))) for i in range(nmax)]
    msgs = [i.to_bytes(8, "little") + rnd.randbytes(MSG_LEN - 8) for i in range(nmax)]
    keys = ctx.ed25519_keys_batch(seeds)
    assert len(set(seeds)) == nmax and len({keys[64 * i:64 * i + 64] for i in range(nmax)}) == nmax and len(set(msgs)) == nmax
    res = {"device": torch.cuda.get_device_name(0), "host_threads": L.load_library().bzk_host_default_threads(), "message_bytes": MSG_LEN, "sizes": []}
    for n in SIZES:
        if n > nmax:
            continue
        k, m, s = keys[:64 * n], msgs[:n], seeds[:n]
        dev, host = alternate(lambda: ctx.ed25519_sign_batch(k, m), lambda: L.host_ed25519_sign_batch(k, m))
        kdev, khost = alternate(lambda: ctx.ed25519_keys_batch(s), lambda: L.host_ed25519_keys_batch(s))
        row = {"n": n,
               "sign": {"device": dict(spread(dev), per_s=n / med(dev)), "host_threads": dict(spread(host), per_s=n / med(host)),
                        "ratio": med(host) / med(dev), "ratio_range": [min(host) / max(dev), max(host) / min(dev)],
                        "kernels_ms": kernel_ms(ctx, lambda: ctx.ed25519_sign_batch(k, m), "ed25519_sign")},
               "keys": {"device": dict(spread(kdev), per_s=n / med(kdev)), "host_threads": dict(spread(khost), per_s=n / med(khost)),
                        "ratio": med(khost) / med(kdev), "ratio_range": [min(khost) / max(kdev), max(khost) / min(kdev)],
                        "kernels_ms": kernel_ms(ctx, lambda: ctx.ed25519_keys_batch(s), "ed25519_keys")}}
        if n == nmax:  # the verifier's kernel over the same rows, three launches
            sig = ctx.ed25519_sign_batch(k, m)
            pks = b"".join(k[64 * i + 32:64 * i + 64] for i in range(n))
            assert ctx.ed25519_verify_batch(pks, m, sig) == b"\x01" * n
            row["verify_kernel_ms"] = [kernel_ms(ctx, lambda: ctx.ed25519_verify_batch(pks, m, sig), "ed25519_verify") for _ in range(3)]
            row["sign_kernel_ms"] = [kernel_ms(ctx, lambda: ctx.ed25519_sign_batch(k, m), "ed25519_sign") for _ in range(3)]
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    for what in ("sign", "keys"):
        wins = [r["n"] for r in res["sizes"] if r[what]["ratio"] >= 1]
        res[what + "_device_stops_losing_at_n"] = min(wins) if wins else None
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
