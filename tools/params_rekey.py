"""The phase-2 step of a ceremony on a bellman `Parameters` file: delta times a fresh secret d (h and l times 1 / d), and the check of such a step.

  python tools/params_rekey.py IN OUT [--d-file FILE] [--host]     re-key IN into OUT; d = os.urandom reduced mod r (never 0), or the 32 bytes of
                                                                   FILE (a little-endian integer, reduced mod r).  d is neither printed nor kept.
  python tools/params_rekey.py --check BEFORE AFTER [--seed-file FILE] [--host]
                                                                   is AFTER a re-key of BEFORE by some d?  exit status 0 yes, 1 no (the report names
                                                                   the array and index); the seed of the check is os.urandom unless FILE gives it -
                                                                   the verdict is only as good as its secrecy from whoever made AFTER.

--host runs on the host's threads (no GPU).  This re-keys delta ALONE: it is one contribution to a ceremony, not a ceremony - a dev-mode CRS whose tau
somebody knows stays unsound whatever is done to delta."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARRAYS = ("the verifying key", "ic", "h", "l", "a", "b_g1", "b_g2", "the array lengths")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs=2, metavar="FILE")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--d-file")
    ap.add_argument("--seed-file")
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    from bazuka_amd import lib as L
    from oracle import pyref as pr
    ctx = None
    if not a.host:
        import torch
        from bazuka_amd import Bzk
        torch.cuda.set_device(0)
        ctx = Bzk(0, torch.cuda.current_stream().cuda_stream)
    try:
        first = open(a.files[0], "rb").read()
        if a.check:
            seed = open(a.seed_file, "rb").read(32) if a.seed_file else os.urandom(32)
            verdict, report = L.bellman_params_rekey_check(ctx, first, open(a.files[1], "rb").read(), seed)
            if verdict == 1:
                print("re-key accepted")
                return 0
            print("re-key REFUSED: %s[%d], code %d" % (ARRAYS[min(report[0], 7)], report[1], report[2]))
            return 1
        if a.d_file:
            d = int.from_bytes(open(a.d_file, "rb").read(32), "little") % pr.R_MOD
            if d == 0:
                print("d is zero mod r", file=sys.stderr)
                return 2
        else:
            d = int.from_bytes(os.urandom(64), "little") % (pr.R_MOD - 1) + 1  # 1 .. r - 1, the bias below 2^-256
        out = L.bellman_params_rekey(ctx, first, pr.fr_to_mont_bytes(d))
        with open(a.files[1], "wb") as f:
            f.write(out)
        print("wrote %s (%d bytes)" % (a.files[1], len(out)))
        return 0
    finally:
        if ctx is not None:
            ctx.close()


if __name__ == "__main__":
    sys.exit(main())
