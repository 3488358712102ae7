#!/usr/bin/env python3
"""Measures wire-form withdrawal verification (bzk_mpn_withdraw_verify_batch), the device SHA3-256 batch (bzk_sha3_256_batch) and withdrawal
admission (bzk_mpn_push_withdraws).  Needs an MI355X: no fallback.

  withdrawals  records/s of bzk_mpn_withdraw_verify_batch at n = 2^10 .. 2^18 records with empty memos (host clock, parsing and copies included)
               against the route available without it: 16 host threads doing, per record, the key decompression (bzk_host_jubjub_decompress),
               the fingerprint (bzk_host_sha3_256 over the payment with its calldata zeroed, bzk_host_scalar_new) and the two Poseidon hashes
               (bzk_host_poseidon), then ONE bzk_jubjub_verify_batch on the device.  The route is given its inputs already cut out of the records
               (the parsing it would also need is not counted against it).  New entry and old route run alternately, three runs each, and the
               ranges are kept.  Up to 2^14 records the host stage is run in full; above, its time is n over the rate measured at 2^14 (it is
               linear in n and would otherwise take most of the run), and only the device part is timed.  The host stage is also given at 16
               times its single-thread rate: the bound a native pool could reach without the interpreter's hand-overs.
  sha3         messages/s of bzk_sha3_256_batch for 2^16 messages of 112 and of 1 000 bytes, against hashlib on one thread.
  admission    wall time of bzk_mpn_push_withdraws for 256 and 4 096 records, with and without a device.
  context      bzk_host_jubjub_verify on 16 threads, the box's rate.

usage: python tools/withdraw_admit_bench.py [--out profiles/mpn_withdraw_verify_batch.json] [--max-log 18]"""
import argparse
import concurrent.futures
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)
sys.path.append(os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bazuka_amd import lib as L  # noqa: E402
from oracle import pyref as pr  # noqa: E402

F = pr.fr_to_mont_bytes
HOST_FULL_MAX = 1 << 14


def pool_map(fn, n, threads):
    step = (n + threads - 1) // threads
    if threads == 1:
        return [fn(0, n)]
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        return list(ex.map(lambda lo: fn(lo, min(n, lo + step)), range(0, n, step)))


def host_stage(items, threads):
    """per record on a thread pool: decompress, fingerprint, H2, H6, calldata comparison.  items: (x, odd, nonce, sig, payment, calldata offset).
    -> (keys n x 64, sign messages n x 32, bytes: bit 0 key decompressed, bit 1 calldata matches)"""
    def run(lo, hi):
        keys, msgs, flags = [], [], bytearray()
        for x, odd, nonce, sig, pay, cd in items[lo:hi]:
            xy = L.host_jubjub_decompress(x, odd)
            fp = L.host_scalar_new(L.host_sha3_256(pay[:cd] + bytes(32) + pay[cd + 32:]))
            nb = F(nonce)
            msgs.append(L.host_poseidon(fp + nb))
            call = L.host_poseidon((xy or bytes(64)) + nb + sig)
            keys.append(xy or bytes(64))
            flags.append((1 if xy else 0) | (2 if call == pay[cd:cd + 32] else 0))
        return b"".join(keys), b"".join(msgs), bytes(flags)
    parts = pool_map(run, len(items), threads)
    return b"".join(p[0] for p in parts), b"".join(p[1] for p in parts), b"".join(p[2] for p in parts)


def spread(v):
    return {"runs_s": v, "min_s": min(v), "max_s": max(v), "median_s": sorted(v)[len(v) // 2]}


def withdrawals(ctx, logs):
    import withdraw_cases as Wd
    base_n = 1 << 12
    recs = Wd.bulk(base_n, 61, pool=192)
    want = L.host_mpn_withdraw_verify_batch(b"".join(recs), base_n)
    import bincode_ref as B
    items = []
    for r in recs:
        v = B.decode(B.MpnWithdraw, r)
        s = v["mpn_sig"]
        items.append((v["mpn_address"]["x"], v["mpn_address"]["odd"], v["mpn_withdraw_nonce"], s["r"]["x"] + s["r"]["y"] + s["s"],
                      Wd.payment_bytes(v), Wd.calldata_offset(v)))
    sigs = b"".join(i[3] for i in items)
    t1 = []
    for _ in range(2):
        a = time.perf_counter()
        host_stage(items[:1024], 1)
        t1.append(time.perf_counter() - a)
    host1_rate = 1024 / min(t1)
    out = {"host_stage_1_thread": {"n": 1024, "runs_s": t1, "per_s": host1_rate}, "sizes": []}
    host16_rate = None
    for k in logs:
        n = 1 << k
        rep = (n + base_n - 1) // base_n
        blob, w = b"".join((recs * rep)[:n]), ((want[0] * rep)[:n], (want[1] * rep)[:32 * n])
        its, sg = (items * rep)[:n], (sigs * rep)[:96 * n]
        assert ctx.mpn_withdraw_verify_batch(blob, n) == w  # also the warm-up
        full = n <= HOST_FULL_MAX
        keys, msgs, flags = host_stage(its, 16) if full else host_stage(its[:base_n], 16)
        if not full:
            keys, msgs, flags = (keys * rep)[:64 * n], (msgs * rep)[:32 * n], (flags * rep)[:n]
        ok = ctx.jubjub_verify_batch(keys, msgs, sg)
        assert bytes(((o & f & 1) | (f & 2)) if f & 1 else 0 for o, f in zip(ok, flags)) == w[0]
        new, host, dev = [], [], []
        for _ in range(3):  # alternating: new entry, old route
            a = time.perf_counter()
            ctx.mpn_withdraw_verify_batch(blob, n)
            new.append(time.perf_counter() - a)
            a = time.perf_counter()
            if full:
                keys, msgs, flags = host_stage(its, 16)
            b = time.perf_counter()
            ctx.jubjub_verify_batch(keys, msgs, sg)
            c = time.perf_counter()
            host.append(b - a)
            dev.append(c - b)
        if full:
            host16_rate = n / sorted(host)[1]
        else:
            host = [n / host16_rate] * 3
        old = [h + d for h, d in zip(host, dev)]
        ideal = [n / (16 * host1_rate) + d for d in dev]
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        row = {"n": n, "withdraw_verify_batch": dict(spread(new), per_s=n / med(new)),
               "route_without": {"host_stage_measured_at_this_n": full, "host_stage_s": spread(host), "verify_batch_s": spread(dev),
                                 "total_s": spread(old), "per_s": n / med(old), "host_share": med(host) / med(old),
                                 "with_ideal_16x_host_pool": {"total_s": spread(ideal), "per_s": n / med(ideal)}},
               "ratio": med(old) / med(new), "ratio_range": [min(old) / max(new), max(old) / min(new)],
               "ratio_with_ideal_16x_host_pool": med(ideal) / med(new)}
        out["sizes"].append(row)
        print(json.dumps(row), flush=True)
    out["host_stage_16_threads_per_s"] = host16_rate
    return out


def sha3(ctx):
    import withdraw_cases as Wd
    rows = []
    for length in (112, 1000):
        n = 1 << 16
        msgs = Wd.messages([length] * 256, length) * (n // 256)
        want = b"".join(hashlib.sha3_256(m).digest() for m in msgs[:256]) * (n // 256)
        assert ctx.sha3_256_batch(msgs, want_scalar=False)[0] == want
        t = []
        for _ in range(5):
            a = time.perf_counter()
            ctx.sha3_256_batch(msgs, want_scalar=False)
            t.append(time.perf_counter() - a)
        a = time.perf_counter()
        for m in msgs[:4096]:
            hashlib.sha3_256(m).digest()
        h = (time.perf_counter() - a) / 4096
        rows.append({"messages": n, "bytes_each": length, "sha3_256_batch_python_binding": dict(spread(t), per_s=n / sorted(t)[2]), "hashlib_1_thread_per_s": 1 / h})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def admission(ctx):
    import withdraw_cases as Wd
    rows = []
    for n in (256, 4096):
        recs = [Wd.signed_withdraw(b"bench acct%d" % i, 1, "", Wd.custom(Wd.MPN_CONTRACT), Wd.ZIESHA, 10 + i, Wd.ZIESHA, i % 3, hasher=Wd._host_hash)
                for i in range(n)]
        blob = b"".join(Wd.enc(r) for r in recs)
        for label, d in (("host", None), ("device", ctx)):
            runs = []
            for _ in range(4):  # the first run warms the context
                w = L.MpnWorld(15, 3)
                w.set_device(d)
                t0 = time.perf_counter()
                ok, acc = w.push_withdraws(blob, n)
                runs.append(time.perf_counter() - t0)
                assert acc == n
                w.close()
            rows.append({"withdrawals": n, "path": label, "runs_s": runs[1:]})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def host_verify_rate():
    import eddsa_cases as E
    n = 1 << 12
    pub, msg, sig = E.bulk(n, 5)

    def run(lo, hi):
        return [L.host_jubjub_verify(pub[64 * i:64 * i + 64], msg[32 * i:32 * i + 32], sig[96 * i:96 * i + 96]) for i in range(lo, hi)]
    pool_map(run, n, 16)
    t = []
    for _ in range(3):
        a = time.perf_counter()
        pool_map(run, n, 16)
        t.append(time.perf_counter() - a)
    return dict(spread(t), n=n, per_s=n / sorted(t)[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpn_withdraw_verify_batch.json"))
    ap.add_argument("--max-log", type=int, default=18)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "withdraw_admit_bench needs a GPU"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    res = {"device": torch.cuda.get_device_name(0)}
    res["withdrawals"] = withdrawals(ctx, [k for k in (10, 12, 14, 16, 18) if k <= a.max_log])
    res["sha3"] = sha3(ctx)
    res["admission"] = admission(ctx)
    res["host_jubjub_verify_16_threads"] = host_verify_rate()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
