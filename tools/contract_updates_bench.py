#!/usr/bin/env python3
"""Measures bzk_contract_updates_check: the device against the same call without a context (the per-lane functions on the host's threads; the
parent commit has no route for this, so that is the baseline).  Needs an MI355X: no fallback.  Host clock, parsing and copies included; device
and host alternate, three runs each unless noted; every device result is compared with the host's.  Records come from the generators of
tests/contract_update_cases.py with the keys and proofs of tests/golden/contract_update_cases.json.

  calls    (a) n FunctionCall updates of one key, n = 64 .. 2^16, beside the bare bzk_groth16_verify_batch on the same proofs and inputs in the
           same process: the difference is what the stages in front of the verifier cost.
  blocks   (b) m transactions of three updates each - 64 deposits at capacity 3, 64 withdrawals at capacity 3, one function call - m = 256,
           1 024, 4 096.  The proofs are well-formed points that do not verify: both sides run every step of the verifier to its verdict.
  kernels  (c) event-pair milliseconds of each new kernel and of the verifier's three (g16k_*: all key groups side by side in one set of
           launches per round; profiles/contract_updates_check.json is the earlier form, g16v_* group after group), in a run of their own.

usage: python tools/contract_updates_bench.py [--out profiles/contract_updates_check.json] [--max-log 16] [--max-m 4096]"""
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

CALL_SIZES = (64, 1024, 4096, 1 << 14, 1 << 16)
BLOCK_SIZES = (256, 1024, 4096)
HOST_RUNS_ABOVE = {1 << 16: 1}   # the host threads need 4.5 s for 2^16 verifying proofs: one run there


def spread(v):
    return {"runs_s": v, "min_s": min(v), "max_s": max(v), "median_s": sorted(v)[len(v) // 2]}


def med(v):
    return sorted(v)[len(v) // 2]


def kernels_of(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    out = {k: {"launches": cnt, "ms": ms} for k, (cnt, ms) in ctx.prof_dump().items() if k.startswith(("upd_", "g16v_", "g16k_"))}
    ctx.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contract_updates_check.json"))
    ap.add_argument("--max-log", type=int, default=16)
    ap.add_argument("--max-m", type=int, default=4096)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "contract_updates_bench needs a GPU"
    torch.cuda.set_device(0)
    import contract_update_cases as K
    fx = K.fixture()
    H = bytes.fromhex
    state0, height0 = K.STATE0, K.HEIGHT0
    stream = torch.cuda.Stream()
    ctx = L.Bzk(0, stream.cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "host_threads": L.load_library().bzk_host_default_threads(), "calls": [], "blocks": []}

    # (a)
    desc = K.fixture_desc(L)
    rec = K.enc(K.repeatable_call(True))
    vk = K.recorded_tables()[2][0]
    one_input = H(fx["repeatable_commit"]) + K.F(height0) + state0 + H(fx["repeatable_aux"]) + state0
    for n in CALL_SIZES:
        if n > 1 << a.max_log:
            continue
        blob, inputs, proofs = rec * n, one_input * n, rec[-387:] * n
        want = bytes([7] * n)
        assert ctx.contract_updates_check(desc, blob, (n,), height0, state0)[0] == want   # also the warm-up
        assert ctx.groth16_verify_batch(vk, inputs, 5, proofs) == bytes([1] * n)
        dev, bare, host = [], [], []
        for run in range(3):
            t0 = time.perf_counter()
            got = ctx.contract_updates_check(desc, blob, (n,), height0, state0)
            t1 = time.perf_counter()
            ctx.groth16_verify_batch(vk, inputs, 5, proofs)
            t2 = time.perf_counter()
            dev.append(t1 - t0)
            bare.append(t2 - t1)
            if run < HOST_RUNS_ABOVE.get(n, 3):
                ref = L.host_contract_updates_check(desc, blob, (n,), height0, state0)
                host.append(time.perf_counter() - t2)
                assert got == ref
        row = {"n": n, "device": dict(spread(dev), per_s=n / med(dev)), "bare_verifier": spread(bare), "host_threads": dict(spread(host), per_s=n / med(host)),
               "added_stages_s": med(dev) - med(bare), "ratio": med(host) / med(dev), "ratio_range": [min(host) / max(dev), max(host) / min(dev)],
               "kernels": kernels_of(ctx, lambda: ctx.contract_updates_check(desc, blob, (n,), height0, state0))}
        res["calls"].append(row)
        print(json.dumps(row), flush=True)

    # (b) both payment functions at capacity 3; the proofs are the repeatable call's: points on their curves that verify nothing here
    desc3 = K.fixture_desc(L, deposit_caps=(3, 3), withdraw_caps=(3, 3))
    proof = rec[-387:]
    deposits = [K.enc(K.crossing_update(i, True)[0])[:-387] + proof for i in range(8)]
    wd = {"circuit_id": 1, "data": ("Withdraw", {"withdraws": [K.withdraw(q, 1) for q in range(64)]}),
          "next_state": {"state_hash": K.X.scalar("bench next"), "state_size": 1}, "prover": bytes(32), "reward": 1, "proof": K.X.zk_proof("bench")}
    withdraws = K.enc(wd)[:-387] + proof
    for m in BLOCK_SIZES:
        if m > a.max_m:
            continue
        blob = b"".join(deposits[j % 8] + withdraws + rec for j in range(m))
        counts = (3,) * m
        ctx.contract_updates_check(desc3, blob, counts, height0, state0)
        dev, host = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            got = ctx.contract_updates_check(desc3, blob, counts, height0, state0)
            t1 = time.perf_counter()
            ref = L.host_contract_updates_check(desc3, blob, counts, height0, state0)
            t2 = time.perf_counter()
            assert got == ref and set(got[0]) <= {6, 7}
            dev.append(t1 - t0)
            host.append(t2 - t1)
        kernels = kernels_of(ctx, lambda: ctx.contract_updates_check(desc3, blob, counts, height0, state0))
        pairing_ms = sum(v["ms"] for k, v in kernels.items() if k.startswith(("g16v_", "g16k_")))
        other_ms = sum(v["ms"] for k, v in kernels.items() if k.startswith("upd_"))
        row = {"m": m, "updates": 3 * m, "payments": 128 * m, "bytes": len(blob), "device": dict(spread(dev), updates_per_s=3 * m / med(dev)),
               "host_threads": dict(spread(host), updates_per_s=3 * m / med(host)), "ratio": med(host) / med(dev),
               "ratio_range": [min(host) / max(dev), max(host) / min(dev)], "kernels": kernels, "verifier_kernels_ms": pairing_ms,
               "other_kernels_ms": other_ms, "non_pairing_share_of_call": 1 - pairing_ms / 1e3 / med(dev),
               "verifier_launches": sum(v["launches"] for k, v in kernels.items() if k.startswith(("g16v_", "g16k_")))}
        res["blocks"].append(row)
        print(json.dumps(row), flush=True)
    wins = [r["m"] for r in res["blocks"] if r["ratio"] >= 1]
    res["blocks_device_stops_losing_at_m"] = min(wins) if wins else None
    wins = [r["n"] for r in res["calls"] if r["ratio"] >= 1]
    res["calls_device_stops_losing_at_n"] = min(wins) if wins else None
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
