"""Measures the batched subgroup checks and what they add to a proving-key load; writes profiles/subgroup_check.json.

  batch   per group and size (2^16, 2^20 points): the device through the host-pointer entry (staging and read-back included), the device through
          the _dev entry (records resident), and the same call with ctx = NULL on the host's threads - alternating, REPS times each, on one machine.
          The records are 4096 distinct multiples of the generator tiled to the size: a lane's work does not depend on its point.
  loader  bzk_params_load_bellman_checked against bzk_params_load_bellman on the 16-tx Update key (L=15, T=3, B=2: 2^20 domain), generated on the
          GPU from a dev seed and written in bellman's format, alternating, each handle freed before the next load.

usage: python tools/subgroup_check_bench.py [--sizes 16,20] [--reps 3] [--no-loader] [--out profiles/subgroup_check.json]"""
import argparse
import json
import os
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
    ap.add_argument("--no-loader", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgroup_check.json"))
    a = ap.parse_args()
    import torch
    from bazuka_amd import Bzk
    from bazuka_amd import lib as L
    from oracle import coracle as co
    torch.cuda.set_device(0)
    bzk = Bzk(0, torch.cuda.current_stream().cuda_stream)
    host_threads = int(os.environ.get("BZK_HOST_THREADS") or 0) or None
    doc = {"device": torch.cuda.get_device_name(0), "host_threads": host_threads or "the CPU quota (host_default_threads)", "reps": a.reps,
           "method": "alternating device (host pointers) / device (_dev) / host threads per repetition, wall clock around the synchronising call; one warm-up call per route",
           "batch": [], "loader": None}
    tiles = {"g1": co.g1_bases(5, 0, 4096), "g2": co.g2_bases(5, 0, 4096)}
    for group in ("g1", "g2"):
        sz = 96 if group == "g1" else 192
        for lg in [int(x) for x in a.sizes.split(",")]:
            n = 1 << lg
            recs = (tiles[group] * (n // 4096 + 1))[:sz * n]
            dev = torch.frombuffer(bytearray(recs), dtype=torch.uint8).cuda()
            ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            warm = min(n, 4096)
            assert bzk.subgroup_check_batch(group, recs[:sz * warm]) == b"\1" * warm
            assert L.host_subgroup_check_batch(group, recs[:sz * warm]) == b"\1" * warm
            bzk.subgroup_check_batch_dev(group, dev, None, warm, ok)
            t = {"device_host_pointers": [], "device_dev_pointers": [], "host_threads": []}
            for _ in range(a.reps):
                dt, got = timed(lambda: bzk.subgroup_check_batch(group, recs))
                assert got == b"\1" * n
                t["device_host_pointers"].append(dt)
                dt, _ = timed(lambda: bzk.subgroup_check_batch_dev(group, dev, None, n, ok))
                assert bool((ok == 1).all())
                t["device_dev_pointers"].append(dt)
                dt, got = timed(lambda: L.host_subgroup_check_batch(group, recs))
                assert got == b"\1" * n
                t["host_threads"].append(dt)
            row = {"group": group, "log2_points": lg, **{k: summary(v) for k, v in t.items()}}
            row["points_per_s_dev_pointers"] = round(n / row["device_dev_pointers"]["median_s"])
            row["host_over_device_host_pointers"] = round(row["host_threads"]["median_s"] / row["device_host_pointers"]["median_s"], 2)
            doc["batch"].append(row)
            print(json.dumps(row), flush=True)
            del dev, ok
    if not a.no_loader:
        from bazuka_amd.worker import DevSetup, dev_toxic
        setup = DevSetup(bzk, {2: dev_toxic("subgroup-bench", 2)})
        r = setup.shape_circuit(2, 15, 3, 2)
        t_gen, (ph, vkb) = timed(lambda: setup.keys(2, 15, 3, 2))
        parts = [bzk.params_read(ph, which) for which in range(6)]
        blob = L.bellman_params_encode(parts[0], vkb[878:], *parts[1:])
        bzk.params_free(ph)
        shape = (r.n_in, r.n_aux, r.view("a_density"), r.view("b_density"))
        counts = {"g1_points": sum(len(parts[k]) for k in (1, 2, 3, 4)) // 96 + r.n_in + 3, "g2_points": len(parts[5]) // 192 + 3}
        t = {"unchecked": [], "checked": []}
        for _ in range(a.reps):
            dt, (h, _) = timed(lambda: bzk.params_load_bellman(blob, *shape))
            bzk.params_free(h)
            t["unchecked"].append(dt)
            dt, (h, _) = timed(lambda: bzk.params_load_bellman_checked(blob, *shape))
            bzk.params_free(h)
            t["checked"].append(dt)
        dt_dev, v_dev = timed(lambda: bzk.bellman_params_check(blob))
        assert v_dev[0] == 1
        doc["loader"] = {"key": "UpdateCircuit(L=15,T=3,B=2): 16 tx, domain 2^20", "file_bytes": len(blob), **counts,
                         "unchecked": summary(t["unchecked"]), "checked": summary(t["checked"]),
                         "check_adds_s": round(statistics.median(t["checked"]) - statistics.median(t["unchecked"]), 6),
                         "bellman_params_check_with_ctx_s": round(dt_dev, 6)}
        print(json.dumps(doc["loader"]), flush=True)
        r.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    bzk.close()


if __name__ == "__main__":
    main()
