"""bzk_groth16_prove_witness against bzk_groth16_prove on the Update circuit, and the coefficient statistics of its matrices.

  python tools/r1cs_eval_bench.py count [lg t b]         CPU only: distinct coefficients, share of +-1 entries, row lengths, resident bytes of
                                                         Update(lg, t, b) (default 15 3 2) from a record_matrices synthesis
  python tools/r1cs_eval_bench.py prove [n] [lg t b]     GPU: n (default 24) pairs of proofs, alternating; the old call runs in a child process on the
                                                         library named by BZK_PARENT_LIB (a build of the parent commit, tools/build_variant.sh) when set,
                                                         and on this build's bzk_groth16_prove in any case; proof bytes compared on every pair
  python tools/r1cs_eval_bench.py trace [lg t b]         GPU: a few proofs of each kind for a `rocprofv3 --kernel-trace --stats` run of its own
  python tools/r1cs_eval_bench.py trace-old [lg t b]     GPU: four proofs by bzk_groth16_prove on the library BZK_LIBBZK names (the parent commit's), for the
                                                         same kind of run with --memory-copy-trace: the three uploads against the lanes' kernels

Every mode prints one JSON line; `prove` also writes it to profiles/r1cs_eval.json when BZK_WRITE_PROFILE=1."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
MONT = (1 << 256) % R_MOD


def fr(x):
    return (x * MONT % R_MOD).to_bytes(32, "little")


def blind(k):
    import hashlib
    return fr(int.from_bytes(hashlib.sha256(b"r1cs_eval_bench %d" % k).digest(), "little") % R_MOD)


def world(L, lg, t, b):
    n_tx = 1 << (2 * b)
    w = L.MpnWorld(lg, t)
    for i in range(2 * n_tx):
        w.add_account(i, b"acct%d" % i, fr(1), 10 ** 12)

    def batch(k):
        for i in range(n_tx):
            w.push_tx(i, n_tx + i, fr(1), 100 + i + k, fr(1), i % 7)
    return w, batch


def count(lg, t, b):
    import numpy as np
    from bazuka_amd import lib as L
    w, batch = world(L, lg, t, b)
    batch(0)
    r = w.update_synthesize(b, fr(99), fr(1), record_matrices=True)
    assert r.satisfied
    out = {"circuit": f"Update({lg},{t},{b})", "n_rows": r.n_constraints, "n_vars": r.n_in + r.n_aux}
    vals = np.concatenate([np.frombuffer(r.raw("val" + x), dtype=np.uint8, count=32 * n).reshape(-1, 32)
                           for x, n in zip("ABC", (r.nnzA, r.nnzB, r.nnzC))])
    v = np.ascontiguousarray(vals).view([("w", "<u8", 4)]).reshape(-1)
    uniq, counts = np.unique(v, return_counts=True)
    one, minus = np.frombuffer(fr(1), dtype=v.dtype)[0], np.frombuffer(fr(R_MOD - 1), dtype=v.dtype)[0]
    pm1 = int(counts[uniq == one].sum() + counts[uniq == minus].sum())
    out.update(nnz=[r.nnzA, r.nnzB, r.nnzC], distinct_coefficients=int(len(uniq)), pm1_entries=pm1, pm1_share=round(pm1 / len(v), 4))
    hist = {}
    for x in "ABC":
        rp = np.frombuffer(r.raw("rp" + x), dtype=np.uint32, count=r.n_constraints + 1).astype(np.int64)
        ln = np.diff(rp)
        hist[x] = {"max": int(ln.max()), "rows_over_12": int((ln > 12).sum()), "terms_in_rows_over_12": int(ln[ln > 12].sum())}
    out["row_lengths"] = hist
    t0 = time.perf_counter()
    mh = L.r1cs_mats_from(r)
    out["host_load_s"] = round(time.perf_counter() - t0, 3)
    info = L.r1cs_mats_info(mh)
    assert info["n_coeffs"] == len(uniq)
    out["resident_bytes"] = info["resident_bytes"]
    out["resident_bytes_per_nnz"] = round(info["resident_bytes"] / len(v), 3)
    t0 = time.perf_counter()
    az, bz, cz, first = L.r1cs_eval(mh, r.raw("z"), True)
    out["host_eval_s"] = round(time.perf_counter() - t0, 3)
    assert first == -1 and az == r.view("az") and bz == r.view("bz") and cz == r.view("cz")
    L.r1cs_mats_free(mh)
    print(json.dumps(out))


def setup(lg, t, b):
    from bazuka_amd import Bzk, lib as L
    ctx = Bzk(0)
    w, batch = world(L, lg, t, b)
    batch(0)
    r = w.update_synthesize(b, fr(99), fr(1), record_matrices=True)
    assert r.satisfied
    csr = [(r.n_constraints, r.raw("rp" + x), r.raw("col" + x), r.raw("val" + x)) for x in "ABC"]
    tox = b"".join(fr(x) for x in (1234567, 2345678, 3456789, 4567891, 5678912))
    ph, _ = ctx.groth16_setup(csr, r.n_in, r.n_aux, tox)
    return ctx, L, w, batch, r, ph


def old_call_child(lg, t, b, n):
    """runs in a child process on the library BZK_LIBBZK names: n proofs by bzk_groth16_prove, one line per proof (ms, hex) after a line 'ready';
    a proof starts when the parent writes a line"""
    prune_for_parent_library()
    ctx, L, w, batch, r, ph = setup(lg, t, b)
    z, az, bz, cz = r.raw("z"), r.raw("az"), r.raw("bz"), r.raw("cz")
    for k in range(3):
        ctx.groth16_prove(ph, z, az, bz, cz, blind(0), blind(1))
    print("ready", flush=True)
    for k in range(n):
        sys.stdin.readline()
        t0 = time.perf_counter()
        p = ctx.groth16_prove(ph, z, az, bz, cz, blind(2 * k), blind(2 * k + 1))
        print(f"{(time.perf_counter() - t0) * 1e3:.4f} {p.hex()}", flush=True)


def prove(n, lg, t, b):
    parent_lib = os.environ.get("BZK_PARENT_LIB")
    child = None
    if parent_lib:
        env = dict(os.environ, BZK_LIBBZK=parent_lib)
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "old-child", str(n), str(lg), str(t), str(b)], env=env,
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    ctx, L, w, batch, r, ph = setup(lg, t, b)
    t0 = time.perf_counter()
    mh = ctx.r1cs_mats_from(r)
    load_s = time.perf_counter() - t0
    info = ctx.r1cs_mats_info(mh)
    z, az, bz, cz = r.raw("z"), r.raw("az"), r.raw("bz"), r.raw("cz")
    for k in range(3):  # warm-up: resident forms, workspaces, the h table
        ctx.groth16_prove(ph, z, az, bz, cz, blind(0), blind(1))
        ctx.groth16_prove_witness(ph, mh, z, blind(0), blind(1))
    if child:
        assert child.stdout.readline().strip() == "ready"
    ms = {"prove_parent": [], "prove": [], "prove_witness": [], "prove_witness_check": []}
    same = True
    for k in range(n):
        rb, sb = blind(2 * k), blind(2 * k + 1)
        got = {}
        if child:
            child.stdin.write("go\n"); child.stdin.flush()
            a, hx = child.stdout.readline().split()
            ms["prove_parent"].append(float(a)); got["prove_parent"] = bytes.fromhex(hx)
        for name, fn in (("prove", lambda: ctx.groth16_prove(ph, z, az, bz, cz, rb, sb)),
                         ("prove_witness", lambda: ctx.groth16_prove_witness(ph, mh, z, rb, sb)),
                         ("prove_witness_check", lambda: ctx.groth16_prove_witness(ph, mh, z, rb, sb, check=True))):
            t0 = time.perf_counter(); got[name] = fn(); ms[name].append((time.perf_counter() - t0) * 1e3)
        same = same and len(set(got.values())) == 1
    if child:
        child.stdin.close(); child.wait()
    out = {"circuit": f"Update({lg},{t},{b})", "n_rows": r.n_constraints, "n_vars": r.n_in + r.n_aux, "pairs": n, "proof_bytes_equal_on_every_pair": same,
           "handle": {"load_s": round(load_s, 3), "resident_bytes": info["resident_bytes"], "distinct_coefficients": info["n_coeffs"],
                      "bytes_per_nnz": round(info["resident_bytes"] / (info["nnzA"] + info["nnzB"] + info["nnzC"]), 3)},
           "ms": {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ms.items() if v}}
    print(json.dumps(out))
    if os.environ.get("BZK_WRITE_PROFILE") == "1":
        with open(os.path.join(ROOT, "profiles", "r1cs_eval.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    assert same


def prune_for_parent_library():
    """a build of the parent commit lacks the calls under test: the binding must not ask for them"""
    import ctypes
    from bazuka_amd import lib as L0
    so = ctypes.CDLL(L0.LIB_PATH)
    for name in [k for k in L0.SIGNATURES if not hasattr(so, k)]:
        del L0.SIGNATURES[name]


def trace_old(lg, t, b):
    """four proofs by bzk_groth16_prove on the library BZK_LIBBZK names (a build of the parent commit), for a trace of the three copies and the lanes"""
    prune_for_parent_library()
    ctx, L, w, batch, r, ph = setup(lg, t, b)
    z, az, bz, cz = r.raw("z"), r.raw("az"), r.raw("bz"), r.raw("cz")
    for k in range(4):
        ctx.groth16_prove(ph, z, az, bz, cz, blind(0), blind(1))
    print(json.dumps({"traced": 4}))


def trace(lg, t, b):
    ctx, L, w, batch, r, ph = setup(lg, t, b)
    mh = ctx.r1cs_mats_from(r)
    z, az, bz, cz = r.raw("z"), r.raw("az"), r.raw("bz"), r.raw("cz")
    for k in range(4):
        ctx.groth16_prove(ph, z, az, bz, cz, blind(0), blind(1))
    for k in range(4):
        ctx.groth16_prove_witness(ph, mh, z, blind(0), blind(1), check=(k == 3))
    print(json.dumps({"traced": 8}))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "count"
    nums = [int(x) for x in sys.argv[2:]]
    if mode == "count":
        count(*(nums or [15, 3, 2]))
    elif mode == "prove":
        prove(nums[0] if nums else 24, *(nums[1:] or [15, 3, 2]))
    elif mode == "old-child":
        old_call_child(nums[1], nums[2], nums[3], nums[0])
    elif mode == "trace":
        trace(*(nums or [15, 3, 2]))
    elif mode == "trace-old":
        trace_old(*(nums or [15, 3, 2]))
    else:
        sys.exit(__doc__)
