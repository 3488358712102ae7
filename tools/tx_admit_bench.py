#!/usr/bin/env python3
"""Measures key decompression on the device (bzk_jubjub_decompress_batch / _dev), wire-form transaction verification (bzk_mpn_tx_verify_batch) and
mempool admission (bzk_mpn_push_txs).  Needs an MI355X: no fallback.

  decompression  keys/s at n = 2^10, 2^14, 2^16, 2^20 from host pointers (copies included, host clock around the synchronising entry) and from device
                 buffers (device events around the enqueue), against bzk_host_jubjub_decompress on 16 threads in the same process (measured on 2^13
                 keys; the rate is reused for the larger sizes); the time of a single launch (n = 64, device buffers).
  transactions   transactions/s of bzk_mpn_tx_verify_batch at the same sizes (host clock, parsing and copies included) against the best route without
                 it: 16 host threads decompressing both keys, then bzk_poseidon_batch with arity 7, then bzk_jubjub_verify_batch, timed stage by
                 stage in the same process; their ratio, and the share of that route spent in host decompression.  The route is given its inputs
                 already cut out of the records (the parsing it would also need is not counted against it).
  admission      wall time of bzk_mpn_push_txs for 256 and 4 096 transactions, with and without a device.
  work decode    bzk_mpn_work_decode of an Update work (two host square roots per transition, rd_pubkey) per transition.
Every shape runs once before it is timed; at least 10 calls or 0.5 s, whichever is longer.

usage: python tools/tx_admit_bench.py [--out profiles/mpn_tx_verify_batch.json] [--max-log 20]"""
import argparse
import concurrent.futures
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


def timed(fn, min_calls=10, min_s=0.5):
    fn()  # warm-up
    t, calls, t0 = [], 0, time.perf_counter()
    while calls < min_calls or time.perf_counter() - t0 < min_s:
        a = time.perf_counter()
        fn()
        t.append(time.perf_counter() - a)
        calls += 1
    t.sort()
    return {"calls": calls, "median_s": t[len(t) // 2], "min_s": t[0], "max_s": t[-1]}


def timed_events(stream, enqueue):
    ev = []

    def call():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        enqueue()
        b.record(stream)
        b.synchronize()
        ev.append(a.elapsed_time(b) / 1e3)
    timed(call)
    ev = sorted(ev[1:])
    return {"calls": len(ev), "median_s": ev[len(ev) // 2], "min_s": ev[0], "max_s": ev[-1]}


def host_decompress(x, odd, n, threads=16):
    """bzk_host_jubjub_decompress for n keys on a thread pool (ctypes releases the interpreter lock during the call; the arguments are offsets into
    two buffers, so that little Python runs between calls): (xy, ok)"""
    import ctypes as C
    lib, step = L.load_library(), (n + threads - 1) // threads
    xb, out = C.create_string_buffer(x, len(x)), C.create_string_buffer(64 * n)
    fn = lib.bzk_host_jubjub_decompress

    def run(lo):
        return bytes(fn(C.byref(xb, 32 * i), odd[i], C.byref(out, 64 * i)) for i in range(lo, min(n, lo + step)))
    if threads == 1:
        return out.raw, run(0)
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        ok = b"".join(ex.map(run, range(0, n, step)))
    return out.raw, ok


def host16_decompress(x, odd, n):
    return host_decompress(x, odd, n, 16)


def dev(b, stream):
    with torch.cuda.stream(stream):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def decompression(ctx, stream, sizes):
    import decompress_cases as D
    base_n = 1 << 13
    x, odd = D.bulk_keys(base_n, 77)
    want = host16_decompress(x, odd, base_n)
    h = timed(lambda: host16_decompress(x, odd, base_n), min_calls=3)
    host_rate = base_n / h["median_s"]
    h1 = timed(lambda: host_decompress(x, odd, base_n, 1), min_calls=3)
    # the pool's rate carries the interpreter's hand-overs between threads; 16 times the single-thread rate is the bound a native pool could reach
    out = {"host_16_threads": dict(h, n=base_n, per_s=host_rate), "host_1_thread": dict(h1, n=base_n, per_s=base_n / h1["median_s"]), "sizes": []}

    def dev_run(n, xs, odds):
        d = [dev(xs, stream), dev(odds, stream)]
        with torch.cuda.stream(stream):
            xy, ok = torch.zeros(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
        stream.synchronize()
        t = timed_events(stream, lambda: ctx.jubjub_decompress_batch_dev(d[0], d[1], n, xy, ok))
        return t, bytes(xy.cpu().numpy().tobytes()), bytes(ok.cpu().numpy().tobytes())

    t, xy, ok = dev_run(64, x[:64 * 32], odd[:64])
    assert (xy, ok) == (want[0][:64 * 64], want[1][:64])
    out["single_launch_64_keys"] = t
    for n in sizes:
        rep = (n + base_n - 1) // base_n
        xs, odds, w = (x * rep)[:32 * n], (odd * rep)[:n], ((want[0] * rep)[:64 * n], (want[1] * rep)[:n])
        assert ctx.jubjub_decompress_batch(xs, odds) == w
        hp = timed(lambda: ctx.jubjub_decompress_batch(xs, odds))
        dv, xy, ok = dev_run(n, xs, odds)
        assert (xy, ok) == w
        out["sizes"].append({"n": n, "host_pointers": dict(hp, per_s=n / hp["median_s"], vs_host_16=n / hp["median_s"] / host_rate),
                             "device_buffers": dict(dv, per_s=n / dv["median_s"], vs_host_16=n / dv["median_s"] / host_rate)})
        print(json.dumps(out["sizes"][-1]), flush=True)
    return out


def transactions(ctx, sizes, host1_rate):
    import decompress_cases as D
    base_n = 1 << 13
    txs = D.tx_bulk(base_n, 55)
    recs = [D.enc_tx(t) for t in txs]
    want = L.host_mpn_tx_verify_batch(b"".join(recs), base_n)
    # the inputs of the route without the new entry, cut out of the records beforehand
    sx, sodd = b"".join(t["src"][0] for t in txs), bytes(t["src"][1] for t in txs)
    dx, dodd = b"".join(t["dst"][0] for t in txs), bytes(t["dst"][1] for t in txs)
    sig = b"".join(t["sig"] for t in txs)
    rows = []
    for n in sizes:
        rep = (n + base_n - 1) // base_n
        blob, w = b"".join((recs * rep)[:n]), ((want[0] * rep)[:n], (want[1] * rep)[:32 * n])
        assert ctx.mpn_tx_verify_batch(blob, n) == w
        new = timed(lambda: ctx.mpn_tx_verify_batch(blob, n))
        kx, kodd = (sx * rep)[:32 * n] + (dx * rep)[:32 * n], (sodd * rep)[:n] + (dodd * rep)[:n]
        rest = [F(t[k]) for t in (txs * rep)[:n] for k in ("nonce", "atok", "amount", "ftok", "fee")]
        sigs = (sig * rep)[:96 * n]
        stage = {"host_decompress": [], "assemble": [], "poseidon_batch": [], "verify_batch": []}

        def route():
            t0 = time.perf_counter()
            xy, kok = host16_decompress(kx, kodd, 2 * n)
            t1 = time.perf_counter()
            dst = xy[64 * n:]
            tup = b"".join(rest[5 * i] + dst[64 * i:64 * i + 64] + rest[5 * i + 1] + rest[5 * i + 2] + rest[5 * i + 3] + rest[5 * i + 4] for i in range(n))
            t2 = time.perf_counter()
            msg = ctx.poseidon_batch(tup, 7)
            t3 = time.perf_counter()
            ok = ctx.jubjub_verify_batch(xy[:64 * n], msg, sigs)
            t4 = time.perf_counter()
            for k, v in zip(stage, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                stage[k].append(v)
            return ok, kok
        ok, kok = route()
        assert bytes(a & b & c for a, b, c in zip(ok, kok[:n], kok[n:])) == w[0]
        for v in stage.values():
            v.clear()
        for _ in range(3 if n <= 1 << 16 else 1):
            route()
        med = {k: sorted(v)[len(v) // 2] for k, v in stage.items()}
        old_s = med["host_decompress"] + med["poseidon_batch"] + med["verify_batch"]  # the Python assembly is not counted against the route
        ideal = 2 * n / (16 * host1_rate)  # host decompression at 16 times the single-thread rate
        ideal_s = ideal + med["poseidon_batch"] + med["verify_batch"]
        rows.append({"n": n, "tx_verify_batch": dict(new, per_s=n / new["median_s"]),
                     "route_without": {"stages_median_s": med, "counted_s": old_s, "per_s": n / old_s,
                                       "host_decompress_share": med["host_decompress"] / old_s,
                                       "with_ideal_16x_host_pool": {"counted_s": ideal_s, "host_decompress_share": ideal / ideal_s}},
                     "ratio": old_s / new["median_s"], "ratio_with_ideal_16x_host_pool": ideal_s / new["median_s"]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def admission(ctx):
    import decompress_cases as D
    rows = []
    for n in (256, 4096):
        txs = [D.signed_tx(b"acct%d" % (i % 64), b"acct%d" % ((i + 1) % 64), 1 + i // 64, 1, 10 + i, 1, i % 3, D._host_hash) for i in range(n)]
        blob = b"".join(D.enc_tx(t) for t in txs)
        for label, d in (("host", None), ("device", ctx)):
            runs = []
            for _ in range(4):  # the first run warms the context
                w = L.MpnWorld(15, 3)
                w.set_device(d)
                t0 = time.perf_counter()
                ok, acc = w.push_txs(blob, n)
                runs.append(time.perf_counter() - t0)
                assert acc == n
                w.close()
            rows.append({"transactions": n, "path": label, "runs_s": runs[1:]})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def work_decode():
    import decompress_cases as D
    import r1cs_scenarios as sc
    w = D.admission_world()
    for s, d, amount, fee in D.TRANSFERS:
        w.push_tx(s, d, D.ZIESHA, amount, D.ZIESHA, fee)
    blob = w.make_work(2, sc.VKS, 10, log4_batches=(1, 1, 2)).encode()
    t = timed(lambda: L.MpnWork.decode(blob))
    return dict(t, transitions=16, per_transition_s=t["median_s"] / 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpn_tx_verify_batch.json"))
    ap.add_argument("--max-log", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tx_admit_bench needs a GPU"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    sizes = [1 << k for k in (10, 14, 16, 20) if k <= a.max_log]
    res = {"device": torch.cuda.get_device_name(0)}
    res["decompression"] = decompression(ctx, stream, sizes)
    res["transactions"] = transactions(ctx, sizes, res["decompression"]["host_1_thread"]["per_s"])
    res["admission"] = admission(ctx)
    res["work_decode"] = work_decode()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
