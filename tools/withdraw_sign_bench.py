#!/usr/bin/env python3
"""Measures the wire-form withdrawal producer: bzk_mpn_withdraws_sign on the device against the same call without a context (the same per-lane
function on the host's threads).  Needs an MI355X: no fallback.

  sizes      records/s at n = 256, 4 096 and 2^16, all records distinct (a key, a nonce and an amount of its own per record; payments of 112
             bytes: no memo, Ziesha ids), host clock, parse, copies and the scatter included; device and host run alternately, three runs each,
             and the ranges are kept.  Every device result is compared with the host's bytes, and the largest one is verified on the device.
  kernels    milliseconds of mpn_withdraw_sign_kernel and of the SHA3 launch in front of it (event pairs around the launches, in a run of their
             own), beside jubjub_sign_kernel over the same number of rows in the same process: the chained kernel against the bare signer.
  crossing   the smallest measured n from which the device stops losing.

usage: python tools/withdraw_sign_bench.py [--out profiles/withdraw_sign_batch.json] [--max-log 16]"""
import argparse
import hashlib
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)

import torch  # noqa: E402

from bazuka_amd import lib as L  # noqa: E402
from oracle import pyref as pr  # noqa: E402

SIZES = (256, 4096, 1 << 16)
ZIESHA = struct.pack("<I", 1)


def spread(v):
    return {"runs_s": v, "min_s": min(v), "max_s": max(v), "median_s": sorted(v)[len(v) // 2]}


def med(v):
    return sorted(v)[len(v) // 2]


def record(key: bytes, i: int) -> bytes:
    """bincode(MpnWithdraw) of key's i-th withdrawal, unsigned: mpn_sig and calldata are zeros"""
    odd = pr.fr_from_mont_bytes(key[32:64]) & 1
    payment = (struct.pack("<Q", 0) + ZIESHA + struct.pack("<I", 0) + bytes(32) + struct.pack("<Q", 32) + hashlib.sha3_256(b"l1 %d" % i).digest() +
               ZIESHA + struct.pack("<Q", 10 ** 6 + i) + ZIESHA + struct.pack("<Q", i % 7))
    return key[:32] + bytes([odd]) + struct.pack("<I", 1 + i) + bytes(96) + payment


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


def kernel_ms(ctx, fn, labels):
    ctx.prof_enable(True)
    ctx.prof_reset()
    fn()
    ms = {k: v for k, (cnt, v) in ctx.prof_dump().items() if k in labels}
    ctx.prof_enable(False)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "withdraw_sign_batch.json"))
    ap.add_argument("--max-log", type=int, default=16)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "withdraw_sign_bench needs a GPU"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    nmax = max(n for n in SIZES if n <= 1 << a.max_log)
    keys = ctx.jubjub_keys_batch([b"withdraw sign bench %d" % i for i in range(nmax)])
    recs = [record(keys[128 * i:128 * i + 128], i) for i in range(nmax)]
    assert len(set(recs)) == nmax and {len(r) for r in recs} == {133 + 112}
    res = {"device": torch.cuda.get_device_name(0), "host_threads": L.load_library().bzk_host_default_threads(), "payment_bytes": 112, "sizes": []}
    for n in SIZES:
        if n > nmax:
            continue
        k, blob = keys[:128 * n], b"".join(recs[:n])
        dev, host = alternate(lambda: ctx.mpn_withdraws_sign(k, blob, n), lambda: L.host_mpn_withdraws_sign(k, blob, n))
        out, ok, fp = ctx.mpn_withdraws_sign(k, blob, n)
        assert ok == b"\x01" * n
        row = {"n": n, "device": dict(spread(dev), per_s=n / med(dev)), "host_threads": dict(spread(host), per_s=n / med(host)),
               "ratio": med(host) / med(dev), "ratio_range": [min(host) / max(dev), max(host) / min(dev)],
               "kernels_ms": [kernel_ms(ctx, lambda: ctx.mpn_withdraws_sign(k, blob, n), ("mpn_withdraw_sign", "sha3_256")) for _ in range(3)],
               "bare_signer_kernel_ms": [kernel_ms(ctx, lambda: ctx.jubjub_sign_batch(k, fp), ("jubjub_sign",)) for _ in range(3)]}
        row["kernel_ratio_to_bare_signer"] = med([r["mpn_withdraw_sign"] for r in row["kernels_ms"]]) / med([r["jubjub_sign"] for r in row["bare_signer_kernel_ms"]])
        if n == nmax:
            assert ctx.mpn_withdraw_verify_batch(out, n) == (b"\x03" * n, fp)
            row["verified_on_device"] = True
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
    wins = [r["n"] for r in res["sizes"] if r["ratio"] >= 1]
    res["device_stops_losing_at_n"] = min(wins) if wins else None
    res["expected_kernel_ratio_by_operation_count"] = 1.7
    res["not_measured"] = ["sizes other than 256, 4096 and 2^16", "payments longer than 112 bytes (more Keccak blocks per record)",
                           "calls of more than one round", "a split of the call's time between parse, copies and scatter"]
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
