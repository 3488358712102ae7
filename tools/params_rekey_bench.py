"""Measures the point scaling behind a Groth16 re-key and the re-key of a resident key; writes profiles/params_rekey.json.

  scale   per size (2^16, 2^20 points): bzk_g1_scale_batch_dev on resident records against bzk_g1_scale_batch with ctx = NULL on the host's threads,
          alternating, REPS times each, on one machine; every device result is compared with the host's.  The records are 4096 distinct multiples
          of the generator tiled to the size, the scalar a seeded random one: a lane's work does not depend on its point.
  kernel  in a run of its own, with event pairs around the launches: the kernel time of the same device calls.
  rekey   bzk_params_rekey on the 16-tx Update key (L=15, T=3, B=2: 2^20 domain), generated on the GPU from a dev seed, REPS times, each new handle
          freed before the next call.

usage: python tools/params_rekey_bench.py [--sizes 16,20] [--reps 3] [--no-rekey] [--out profiles/params_rekey.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def summary(xs):
    return {"median_s": round(statistics.median(xs), 6), "min_s": round(min(xs), 6), "max_s": round(max(xs), 6), "runs": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-rekey", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "params_rekey.json"))
    a = ap.parse_args()
    import torch
    from bazuka_amd import Bzk
    from bazuka_amd import lib as L
    from oracle import coracle as co
    from oracle import pyref as pr
    torch.cuda.set_device(0)
    bzk = Bzk(0, torch.cuda.current_stream().cuda_stream)
    k = pr.fr_to_mont_bytes(random.Random(20241).randrange(1, pr.R_MOD))
    doc = {"device": torch.cuda.get_device_name(0), "host_threads": L.load_library().bzk_host_default_threads(), "reps": a.reps,
           "method": "alternating device (_dev, records resident) / host threads (ctx = NULL) per repetition, wall clock around the synchronising call; "
                     "one warm-up call per route; kernel time from event pairs in a run of its own",
           "scale": [], "rekey": None}
    tile = co.g1_bases(5, 0, 4096)
    for lg in [int(x) for x in a.sizes.split(",")]:
        n = 1 << lg
        recs = (tile * (n // 4096 + 1))[:96 * n]
        dev = torch.frombuffer(bytearray(recs), dtype=torch.uint8).cuda()
        out = torch.zeros(96 * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        warm = min(n, 4096)
        bzk.g1_scale_batch_dev(dev, warm, k, out, None)
        assert bytes(out[:96 * warm].cpu().numpy().tobytes()) == L.g1_scale_batch(None, recs[:96 * warm], k)[0]
        t = {"device_dev_pointers": [], "host_threads": []}
        for _ in range(a.reps):
            dt, _ = timed(lambda: bzk.g1_scale_batch_dev(dev, n, k, out, None))
            t["device_dev_pointers"].append(dt)
            got = bytes(out.cpu().numpy().tobytes())
            dt, (want, inf) = timed(lambda: L.g1_scale_batch(None, recs, k))
            t["host_threads"].append(dt)
            assert got == want and inf == bytes(n)
        # the kernel alone: event pairs around the launches, in a run of its own
        bzk.prof_filter("g1_scale")
        bzk.prof_enable(True)
        kern = []
        for _ in range(a.reps):
            bzk.prof_reset()
            bzk.g1_scale_batch_dev(dev, n, k, out, None)
            launches, ms = bzk.prof_query("g1_scale")
            kern.append(ms / 1e3)
        bzk.prof_enable(False)
        bzk.prof_filter(None)
        row = {"log2_points": lg, **{name: summary(v) for name, v in t.items()}, "kernel": summary(kern)}
        row["points_per_s_device"] = round(n / row["device_dev_pointers"]["median_s"])
        row["host_over_device"] = round(row["host_threads"]["median_s"] / row["device_dev_pointers"]["median_s"], 2)
        doc["scale"].append(row)
        print(json.dumps(row), flush=True)
        del dev, out
    if not a.no_rekey:
        from bazuka_amd.worker import DevSetup, dev_toxic
        setup = DevSetup(bzk, {2: dev_toxic("rekey-bench", 2)})
        t_gen, (ph, vkb) = timed(lambda: setup.keys(2, 15, 3, 2))
        sizes = [len(bzk.params_read(ph, which)) for which in range(6)]
        ts = []
        for _ in range(a.reps):
            dt, (pn, vk870) = timed(lambda: bzk.params_rekey(ph, k))
            ts.append(dt)
            assert vk870[:580] == vkb[:580] and vk870[580:] != vkb[580:870]
            bzk.params_free(pn)
        doc["rekey"] = {"key": "UpdateCircuit(L=15,T=3,B=2): 16 tx, domain 2^20", "h_points": sizes[1] // 96, "l_points": sizes[2] // 96,
                        "copied_bytes": sizes[3] + sizes[4] + sizes[5], "setup_s": round(t_gen, 3), "params_rekey": summary(ts)}
        print(json.dumps(doc["rekey"]), flush=True)
        bzk.params_free(ph)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    bzk.close()


if __name__ == "__main__":
    main()
