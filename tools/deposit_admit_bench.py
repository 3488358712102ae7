#!/usr/bin/env python3
"""Measures batched Ed25519 verification (bzk_ed25519_verify_batch), wire-form deposit verification (bzk_mpn_deposit_verify_batch) and deposit
admission (bzk_mpn_push_deposits).  Needs an MI355X: no fallback.

  ed25519    signatures/s of bzk_ed25519_verify_batch at n = 2^10 .. 2^18 (messages of 117 bytes, a deposit's signed form; host clock, copies
             included) against the same per-lane code on 16 host threads (ctx = NULL) - the only other Ed25519 route the library has.  Device and
             host run alternately, three runs each, and the ranges are kept.  Every device verdict vector is compared with the host's.
  deposits   the same for bzk_mpn_deposit_verify_batch (parsing and the address decompression included on both sides); the 2^18 row crosses
             three chunk ends of 2^16 records.
  crossover  n = 2^3 .. 2^11: the smallest batch from which the device stops losing to the 16 host threads.
  admission  wall time of bzk_mpn_push_deposits for 256 and 4 096 records, with and without a device.

usage: python tools/deposit_admit_bench.py [--out profiles/mpn_deposit_verify_batch.json] [--max-log 18]"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bazuka_amd import lib as L  # noqa: E402

POOL = 64


def spread(v):
    return {"runs_s": v, "min_s": min(v), "max_s": max(v), "median_s": sorted(v)[len(v) // 2]}


def med(v):
    return sorted(v)[len(v) // 2]


def alternate(dev_fn, host_fn, runs=3):
    dev, host = [], []
    for _ in range(runs):
        a = time.perf_counter()
        dev_fn()
        b = time.perf_counter()
        host_fn()
        c = time.perf_counter()
        dev.append(b - a)
        host.append(c - b)
    return dev, host


def row_of(n, dev, host):
    return {"n": n, "device": dict(spread(dev), per_s=n / med(dev)), "host_16_threads": dict(spread(host), per_s=n / med(host)),
            "ratio": med(host) / med(dev), "ratio_range": [min(host) / max(dev), max(host) / min(dev)]}


def pool_records():
    """POOL signed deposits (empty memo, a Custom contract id: 149 signed bytes) and, for each, a copy with the amount changed"""
    import ed25519_cases as E
    good = [E.signed_deposit(b"bench wallet %d" % i, E.account_address(i % E.N_ACC), "", E.custom(E.MPN_CONTRACT), E.ZIESHA, 10 + i, E.ZIESHA, i % 3)
            for i in range(POOL)]
    bad = []
    for r in good:
        m = copy.deepcopy(r)
        m["payment"]["amount"]["amount"] += 1
        bad.append(m)
    return good, bad


def cycle(items, n):
    return (items * ((n + len(items) - 1) // len(items)))[:n]


def ed25519(ctx, good, bad, sizes):
    import ed25519_cases as E
    triples = []
    for i in range(POOL):  # every fourth signature does not verify
        r = bad[i] if i % 4 == 3 else good[i]
        triples.append((r["payment"]["src"], E.unsigned_bytes(r), r["payment"]["sig"]))
    rows = []
    for n in sizes:
        t = cycle(triples, n)
        pks, msgs, sigs = b"".join(x[0] for x in t), [x[1] for x in t], b"".join(x[2] for x in t)
        want = L.host_ed25519_verify_batch(pks, msgs, sigs)
        assert ctx.ed25519_verify_batch(pks, msgs, sigs) == want == bytes(cycle([0 if i % 4 == 3 else 1 for i in range(POOL)], n))  # also the warm-up
        dev, host = alternate(lambda: ctx.ed25519_verify_batch(pks, msgs, sigs), lambda: L.host_ed25519_verify_batch(pks, msgs, sigs))
        rows.append(row_of(n, dev, host))
        print(json.dumps({"ed25519": rows[-1]}), flush=True)
    return rows


def deposits(ctx, good, bad, sizes):
    import ed25519_cases as E
    recs = [E.enc(bad[i] if i % 4 == 3 else good[i]) for i in range(POOL)]
    rows = []
    for n in sizes:
        blob = b"".join(cycle(recs, n))
        want = L.host_mpn_deposit_verify_batch(blob, n)
        assert want[0] == bytes(cycle([2 if i % 4 == 3 else 3 for i in range(POOL)], n))
        assert ctx.mpn_deposit_verify_batch(blob, n) == want  # also the warm-up
        dev, host = alternate(lambda: ctx.mpn_deposit_verify_batch(blob, n), lambda: L.host_mpn_deposit_verify_batch(blob, n))
        rows.append(row_of(n, dev, host))
        print(json.dumps({"deposits": rows[-1]}), flush=True)
    return rows


def admission(ctx, good):
    import ed25519_cases as E
    rows = []
    for n in (256, 4096):
        blob = b"".join(cycle([E.enc(r) for r in good], n))
        for label, d in (("host", None), ("device", ctx)):
            runs = []
            for _ in range(4):  # the first run warms the context
                w = L.MpnWorld(15, 3)
                w.set_device(d)
                t0 = time.perf_counter()
                ok, acc = w.push_deposits(blob, n)
                runs.append(time.perf_counter() - t0)
                assert acc == n
                w.close()
            rows.append({"deposits": n, "path": label, "runs_s": runs[1:]})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpn_deposit_verify_batch.json"))
    ap.add_argument("--max-log", type=int, default=18)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "deposit_admit_bench needs a GPU"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    good, bad = pool_records()
    sizes = [1 << k for k in (10, 14, 16, 18) if k <= a.max_log]
    res = {"device": torch.cuda.get_device_name(0), "host_threads": L.load_library().bzk_host_default_threads()}
    res["ed25519"] = ed25519(ctx, good, bad, sizes)
    res["deposits"] = deposits(ctx, good, bad, sizes)
    small = ed25519(ctx, good, bad, [1 << k for k in range(3, 12)])
    wins = [r["n"] for r in small if r["ratio"] >= 1]
    res["crossover"] = {"sizes": small, "device_stops_losing_at_n": min(wins) if wins else None}
    res["admission"] = admission(ctx, good)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
