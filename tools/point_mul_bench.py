"""Measures n points times n scalars on G1 and G2 against the one-scalar call, and one contribution to a powers-of-tau accumulator; writes
profiles/point_mul_batch.json.

  mul       per size (2^16, 2^20 points), in ONE process: bzk_g1_mul_batch_dev and bzk_g2_mul_batch_dev on resident records and scalars, and
            bzk_g1_scale_batch_dev on the same G1 records (the yardstick: the same 128 doublings, fewer additions, one scalar for all lanes), one
            warm-up call and REPS timed calls each, wall clock around the synchronising call; then the ctx = NULL route of the two new calls on the
            host's threads, HOST_REPS times.  Every device result of the first timed call is compared with the host's.  The records are 4096 distinct
            multiples of the generator tiled to the size, the scalars seeded uniform values below r.
  kernel    in a run of its own, with event pairs around the launches: the kernel time of the multiplication launches of the same device calls.
  ptau      one bzk_ptau_contribute with a context on the trivial accumulator of log_m = 20 (host pointers: 4 x 2^20 G1 and 2^20 G2 points staged in
            rounds), REPS times.

usage: python tools/point_mul_bench.py [--sizes 16,20] [--reps 5] [--host-reps 5] [--ptau-log-m 20] [--no-ptau] [--out profiles/point_mul_batch.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def summary(xs):
    return {"median_s": round(statistics.median(xs), 6), "min_s": round(min(xs), 6), "max_s": round(max(xs), 6), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--ptau-log-m", type=int, default=20)
    ap.add_argument("--no-ptau", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_mul_batch.json"))
    a = ap.parse_args()
    import torch
    from bazuka_amd import Bzk
    from bazuka_amd import lib as L
    from oracle import coracle as co
    from oracle import pyref as pr
    from util import rand_scalars_bytes
    torch.cuda.set_device(0)
    bzk = Bzk(0, torch.cuda.current_stream().cuda_stream)
    k1 = pr.fr_to_mont_bytes(0x5eed5eed5eed5eed5eed5eed5eed5eed5eed5eed5eed5eed % pr.R_MOD)
    doc = {"device": torch.cuda.get_device_name(0), "host_threads": L.load_library().bzk_host_default_threads(), "reps": a.reps,
           "host_reps": a.host_reps,
           "method": "one process; per call one warm-up and `reps` timed calls, wall clock around the synchronising call (_dev forms, records and "
                     "scalars resident); host threads (ctx = NULL) `host_reps` calls; kernel time from event pairs in a run of its own",
           "mul": [], "ptau": None}
    tiles = {"g1": co.g1_bases(5, 0, 4096), "g2": co.g2_bases(5, 0, 4096)}
    size = {"g1": 96, "g2": 192}
    for lg in [int(x) for x in a.sizes.split(",")]:
        n = 1 << lg
        scal = rand_scalars_bytes(n, seed=lg)
        dk = torch.frombuffer(bytearray(scal), dtype=torch.uint8).cuda()
        row = {"log2_points": lg}
        for g in ("g1", "g2"):
            sz = size[g]
            recs = (tiles[g] * (n // 4096 + 1))[:sz * n]
            dev = torch.frombuffer(bytearray(recs), dtype=torch.uint8).cuda()
            out = torch.zeros(sz * n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            calls = {g + "_mul_batch_dev": lambda: bzk.mul_batch_dev(g, dev, dk, n, out, None)}
            if g == "g1":
                calls["g1_scale_batch_dev"] = lambda: bzk.g1_scale_batch_dev(dev, n, k1, out, None)
            got = None
            for name, call in calls.items():
                call()  # warm-up
                ts = []
                for rep in range(a.reps):
                    dt, _ = timed(call)
                    ts.append(dt)
                    if rep == 0 and name.endswith("mul_batch_dev"):
                        got = bytes(out.cpu().numpy().tobytes())
                row[name] = summary(ts)
            # the kernel alone: event pairs around the multiplication launches, in a run of its own
            bzk.prof_filter(g + "_pmul")
            bzk.prof_enable(True)
            kern = []
            for _ in range(a.reps):
                bzk.prof_reset()
                bzk.mul_batch_dev(g, dev, dk, n, out, None)
                launches, ms = bzk.prof_query(g + "_pmul")
                kern.append(ms / 1e3)
            bzk.prof_enable(False)
            bzk.prof_filter(None)
            row[g + "_pmul_kernel"] = summary(kern)
            ts = []
            for rep in range(a.host_reps):
                dt, (want, inf) = timed(lambda: L.mul_batch(None, g, recs, scal))
                ts.append(dt)
                if rep == 0:
                    assert got == want, g
            row[g + "_host_threads"] = summary(ts)
            row[g + "_points_per_s_device"] = round(n / row[g + "_mul_batch_dev"]["median_s"])
            row[g + "_host_over_device"] = round(row[g + "_host_threads"]["median_s"] / row[g + "_mul_batch_dev"]["median_s"], 2)
            del dev, out
        row["g1_mul_over_g1_scale"] = round(row["g1_mul_batch_dev"]["median_s"] / row["g1_scale_batch_dev"]["median_s"], 3)
        row["g2_mul_over_g1_mul"] = round(row["g2_mul_batch_dev"]["median_s"] / row["g1_mul_batch_dev"]["median_s"], 3)
        doc["mul"].append(row)
        print(json.dumps(row), flush=True)
    if not a.no_ptau:
        lg = a.ptau_log_m
        trivial = L.ptau_init(lg)
        secrets = b"".join(pr.fr_to_mont_bytes(x) for x in (3 ** 150 % pr.R_MOD, 5 ** 100 % pr.R_MOD, 7 ** 90 % pr.R_MOD))
        bzk.ptau_contribute(L.ptau_init(8), secrets)  # warm-up
        ts = []
        for _ in range(a.reps):
            dt, (acc, key) = timed(lambda: bzk.ptau_contribute(trivial, secrets))
            ts.append(dt)
        assert key == L.ptau_contribute(None, L.ptau_init(1), secrets)[1]
        doc["ptau"] = {"log_m": lg, "bytes": len(trivial), "g1_points": 4 * (1 << lg) - 1, "g2_points": (1 << lg) + 1, "contribute": summary(ts)}
        print(json.dumps(doc["ptau"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    bzk.close()


if __name__ == "__main__":
    main()
