#!/usr/bin/env python3
"""Measures the batched signature verifier (bzk_jubjub_verify_batch / _dev) and the withdraw builder that uses it.  Needs an MI355X: no fallback.

  throughput   n = 64, 4 096, 2^16, 2^20 from host pointers (copies included, host clock around the synchronising entry) and from device buffers
               (device events around the enqueue), against bzk_host_jubjub_verify on 16 threads in the same process (measured on 2^14 entries; the
               rate is reused for the larger sizes).  Every size runs once before it is timed; at least 20 calls or 0.5 s, whichever is longer.
  builder      wall time of bzk_mpn_make_work (withdraw) on a world with set_device at 64, 256, 1 024 queued wallet-style withdrawals.  With
               --builder-only the script uses nothing newer than bzk_mpn_set_device, so the same file measures an older checkout of the package
               (PYTHONPATH) for an A/B comparison.

usage: python tools/eddsa_bench.py [--out profiles/eddsa_verify_batch.json] [--builder-only] [--no-builder] [--repeat 3]"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # behind PYTHONPATH: an older checkout of the package named there wins (--builder-only A/B)
sys.path.append(os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bazuka_amd import lib as L  # noqa: E402
from oracle import pyref as pr  # noqa: E402

F = pr.fr_to_mont_bytes
ZIESHA = F(1)


def timed(fn, min_calls=20, min_s=0.5):
    fn()  # warm-up
    t, calls, t0 = [], 0, time.perf_counter()
    while calls < min_calls or time.perf_counter() - t0 < min_s:
        a = time.perf_counter()
        fn()
        t.append(time.perf_counter() - a)
        calls += 1
    t.sort()
    return {"calls": calls, "median_s": t[len(t) // 2], "min_s": t[0], "max_s": t[-1]}


def throughput(ctx, stream):
    import eddsa_cases as E
    base_n = 1 << 14
    pub, msg, sig = E.bulk(base_n, 99)
    want = E.host_verdicts(pub, msg, sig)
    lib = L.load_library()

    def host16():
        step = base_n // 16

        def run(lo):
            return sum(lib.bzk_host_jubjub_verify(pub[64 * i:64 * i + 64], msg[32 * i:32 * i + 32], sig[96 * i:96 * i + 96]) for i in range(lo, lo + step))
        with concurrent.futures.ThreadPoolExecutor(16) as ex:
            return sum(ex.map(run, range(0, base_n, step)))
    h = timed(host16, min_calls=3, min_s=0.5)
    host_rate = base_n / h["median_s"]
    out = {"host_16_threads": dict(h, n=base_n, per_s=host_rate), "sizes": []}
    for n in (64, 4096, 1 << 16, 1 << 20):
        rep = (n + base_n - 1) // base_n
        p, m, s, w = (pub * rep)[:64 * n], (msg * rep)[:32 * n], (sig * rep)[:96 * n], (want * rep)[:n]
        assert ctx.jubjub_verify_batch(p, m, s) == w
        hp = timed(lambda: ctx.jubjub_verify_batch(p, m, s))
        with torch.cuda.stream(stream):
            d = [torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda() for x in (p, m, s)]
            ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        stream.synchronize()
        ev = []

        def dev_call():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            ctx.jubjub_verify_batch_dev(d[0], d[1], d[2], n, ok)
            b.record(stream)
            b.synchronize()
            ev.append(a.elapsed_time(b) / 1e3)
        timed(dev_call)
        assert bytes(ok.cpu().numpy().tobytes()) == w
        ev = sorted(ev[1:])
        dv = {"calls": len(ev), "median_s": ev[len(ev) // 2], "min_s": ev[0], "max_s": ev[-1]}
        out["sizes"].append({"n": n, "host_pointers": dict(hp, per_s=n / hp["median_s"], vs_host_16=n / hp["median_s"] / host_rate),
                             "device_buffers": dict(dv, per_s=n / dv["median_s"], vs_host_16=n / dv["median_s"] / host_rate)})
        print(json.dumps(out["sizes"][-1]), flush=True)
    return out


def builder(ctx, repeat):
    import r1cs_scenarios as sc
    rows = []
    for n, lb in ((64, 3), (256, 4), (1024, 5)):
        runs = []
        for _ in range(repeat + 1):  # the first run warms the context (tables, workspace)
            w = L.MpnWorld(15, 3)
            w.set_device(ctx)
            idx = [(i * 7919 + 3) % (4 ** 15) for i in range(n)]
            for i, a in enumerate(idx):
                w.add_account(a, b"acct%d" % i, ZIESHA, 10 ** 9)
            for i in range(n):
                w.push_withdraw(idx[i], ZIESHA, 10 + i, ZIESHA, i % 3)
            t0 = time.perf_counter()
            work = w.make_work(1, sc.VKS, 12, log4_batches=(1, lb, 1))
            runs.append(time.perf_counter() - t0)
            del work
            w.close()
        rows.append({"withdrawals": n, "runs_s": runs[1:]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eddsa_verify_batch.json"))
    ap.add_argument("--builder-only", action="store_true")
    ap.add_argument("--no-builder", action="store_true")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eddsa_bench needs a GPU"
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "package": os.path.dirname(os.path.abspath(L.__file__))}
    if not a.builder_only:
        res["throughput"] = throughput(ctx, stream)
    if not a.no_builder:
        res["builder"] = builder(ctx, a.repeat)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
