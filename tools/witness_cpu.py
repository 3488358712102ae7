#!/usr/bin/env python3
"""Host CPU-seconds per witness (time.process_time, one generator thread) of the three synthesis modes - plain, BZK_SYNTH_DEFER and
BZK_SYNTH_DEFER_SIG - on update_15_3_2 (16 transitions) and withdraw_15_3_3 (64).  CPU only: nothing here touches a device.

usage: python tools/witness_cpu.py [repeats=5]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import r1cs_scenarios as S  # noqa: E402
from bazuka_amd import lib as L  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = {}
    for name in ("update_15_3_2", "withdraw_15_3_3"):
        dec = L.MpnWork.decode(S.make_work(name))
        row = {}
        for mode, kw in (("plain", False), ("defer", True), ("defer_sig", "sig")):
            dec.synthesize(S.PROVER, threads=1, defer=kw).free()  # warm: the program of a shape is recorded once per process
            ts = []
            for _ in range(reps):
                t0 = time.process_time()
                r = dec.synthesize(S.PROVER, threads=1, defer=kw)
                ts.append(time.process_time() - t0)
                r.free()
            row[mode] = round(min(ts), 4)
        row["defer_sig/defer"] = round(row["defer_sig"] / row["defer"], 3)
        out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
