#!/usr/bin/env python3
"""Measures the wire-form L1 transaction entries: bzk_l1_tx_verify_batch, bzk_block_bodies_check and the lone bzk_sha3_merkle_roots.  Needs an
MI355X: no fallback.

  tx_verify  records/s of bzk_l1_tx_verify_batch (verdicts and hashes) at n = 2^10, 2^14, 2^16 RegularSend records of one entry, every fourth
             with a wrong signature (host clock, parsing and copies included), against the same per-lane code on 16 host threads (ctx = NULL):
             the parent has no route for this arm, so that path is the baseline.  Device and host run alternately, three runs each, and the
             ranges are kept.  Every device result is compared with the host's.
  bodies     the same for bzk_block_bodies_check: 1 block of 4 096 transactions (a lone tree: `depth` dependent launches) and 256 blocks of 256.
  crossover  n = 2^3 .. 2^11 of tx_verify: the smallest batch from which the device stops losing to the 16 host threads.
  lone_tree  bzk_sha3_merkle_roots for one tree of 16, 256 and 4 096 leaves: the latency-bound case.
  long       a batch of 1 024 records with and without one CreateContract record of about 1 MB in it: the lane that holds it keeps its
             wavefront for some 8 000 SHA-512 blocks.

usage: python tools/l1_admit_bench.py [--out profiles/l1_block_check.json]"""
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


def row_of(n, dev, host, **more):
    return dict(more, n=n, device=dict(spread(dev), per_s=n / med(dev)), host_16_threads=dict(spread(host), per_s=n / med(host)),
                ratio=med(host) / med(dev), ratio_range=[min(host) / max(dev), max(host) / min(dev)])


def cycle(items, n):
    return (items * ((n + len(items) - 1) // len(items)))[:n]


def pool_records():
    """POOL signed RegularSend records of one entry; every fourth carries a wrong signature"""
    import l1_tx_cases as X
    recs = []
    for i in range(POOL):
        r = X.enc(X.regular_send(b"bench wallet %d" % i, "payment %d" % i, nonce=i))
        recs.append(X.flip(r, len(r) - 9) if i % 4 == 3 else r)
    return recs


def tx_verify(ctx, recs, sizes, key="tx_verify"):
    rows = []
    for n in sizes:
        blob = b"".join(cycle(recs, n))
        want = L.host_l1_tx_verify_batch(blob, n)
        assert want[0] == bytes(cycle([0 if i % 4 == 3 else 1 for i in range(POOL)], n))
        assert ctx.l1_tx_verify_batch(blob, n) == want  # also the warm-up
        dev, host = alternate(lambda: ctx.l1_tx_verify_batch(blob, n), lambda: L.host_l1_tx_verify_batch(blob, n))
        rows.append(row_of(n, dev, host, record_bytes=len(blob) // n))
        print(json.dumps({key: rows[-1]}), flush=True)
    return rows


def bodies(ctx, recs):
    rows = []
    for blocks, per in ((1, 4096), (256, 256)):
        n = blocks * per
        blob, counts = b"".join(cycle(recs, n)), [per] * blocks
        want = L.host_block_bodies_check(blob, counts)
        assert want[0] == bytes(blocks)  # every body holds a wrong signature
        assert ctx.block_bodies_check(blob, counts) == want  # also the warm-up
        dev, host = alternate(lambda: ctx.block_bodies_check(blob, counts), lambda: L.host_block_bodies_check(blob, counts))
        rows.append(row_of(n, dev, host, blocks=blocks, transactions_per_block=per))
        print(json.dumps({"bodies": rows[-1]}), flush=True)
    return rows


def lone_tree(ctx):
    import hashlib
    rows = []
    for n in (16, 256, 4096):
        leaves = b"".join(hashlib.sha3_256(b"leaf %d" % i).digest() for i in range(n))
        want = L.host_sha3_merkle_roots(leaves, [n])
        assert ctx.sha3_merkle_roots(leaves, [n]) == want
        dev, host = alternate(lambda: ctx.sha3_merkle_roots(leaves, [n]), lambda: L.host_sha3_merkle_roots(leaves, [n]), runs=5)
        rows.append(row_of(n, dev, host))
        print(json.dumps({"lone_tree": rows[-1]}), flush=True)
    return rows


def long_record(ctx, recs):
    import l1_tx_cases as X
    data = ("CreateContract", {"contract": X.zk_contract(False), "money": X.money(1), "state": None})
    pad = X.RECORD_MAX - 64 - len(X.enc(X.sign_tx(b"big wallet", X.tx_of(data, memo=""))))
    big = X.enc(X.sign_tx(b"big wallet", X.tx_of(data, memo="z" * pad)))  # 64 bytes under the limit of 2^20
    n = 1024
    plain = cycle(recs, n)
    rows = []
    for label, batch in (("1024 short records", plain), ("1023 short records and one of %d bytes" % len(big), plain[:500] + [big] + plain[501:])):
        blob = b"".join(batch)
        want = L.host_l1_tx_verify_batch(blob, n)
        assert ctx.l1_tx_verify_batch(blob, n) == want and (batch is plain or want[0][500] == 1)
        dev, host = alternate(lambda: ctx.l1_tx_verify_batch(blob, n), lambda: L.host_l1_tx_verify_batch(blob, n))
        rows.append(row_of(n, dev, host, batch=label))
        print(json.dumps({"long": rows[-1]}), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1_block_check.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "l1_admit_bench needs a GPU"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    recs = pool_records()
    res = {"device": torch.cuda.get_device_name(0), "host_threads": L.load_library().bzk_host_default_threads()}
    res["tx_verify"] = tx_verify(ctx, recs, [1 << 10, 1 << 14, 1 << 16])
    res["bodies"] = bodies(ctx, recs)
    small = tx_verify(ctx, recs, [1 << k for k in range(3, 12)], key="crossover")
    wins = [r["n"] for r in small if r["ratio"] >= 1]
    res["crossover"] = {"sizes": small, "device_stops_losing_at_n": min(wins) if wins else None}
    res["lone_tree"] = lone_tree(ctx)
    res["long"] = long_record(ctx, recs)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
