"""A powers-of-tau accumulator (phase 1 of a ceremony) as this library's flat blob: make the trivial one, contribute to one, check one.

  python tools/ptau.py init LOG_M OUT                               the trivial accumulator for m = 2^LOG_M (1 .. 24): every entry a generator
  python tools/ptau.py contribute IN OUT KEY [--secrets-file FILE] [--host]
                                                                    multiply IN's tau, alpha, beta by fresh secrets into OUT and write the
                                                                    contribution's public key (tau G2 | alpha G2 | beta G2, 576 bytes) to KEY.  The
                                                                    secrets come from os.urandom reduced mod r (never 0), or from the 96 bytes of
                                                                    FILE (three little-endian integers, reduced mod r); they are neither printed
                                                                    nor kept.
  python tools/ptau.py check AFTER [--before BEFORE --key KEY] [--seed-file FILE] [--host]
                                                                    is AFTER a well-formed accumulator and, with --before and --key, one
                                                                    contribution on top of BEFORE?  exit status 0 yes, 1 no (the report names the
                                                                    array and index); the seed of the check is os.urandom unless FILE gives it -
                                                                    the verdict is only as good as its secrecy from whoever made AFTER.

--host runs on the host's threads (no GPU).  This is the arithmetic of a contribution and of its check, not a ceremony client: there is no proof of
knowledge of the key's exponents, no transcript hash, and the multiplier is not hardened against timing."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARRAYS = ("the header or the lengths", "tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2", "the key")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("init")
    p.add_argument("log_m", type=int)
    p.add_argument("out")
    p = sub.add_parser("contribute")
    p.add_argument("inp", metavar="IN")
    p.add_argument("out")
    p.add_argument("key")
    p.add_argument("--secrets-file")
    p.add_argument("--host", action="store_true")
    p = sub.add_parser("check")
    p.add_argument("after")
    p.add_argument("--before")
    p.add_argument("--key")
    p.add_argument("--seed-file")
    p.add_argument("--host", action="store_true")
    a = ap.parse_args()
    from bazuka_amd import lib as L
    from oracle import pyref as pr
    if a.cmd == "init":
        blob = L.ptau_init(a.log_m)
        with open(a.out, "wb") as f:
            f.write(blob)
        print("wrote %s (%d bytes)" % (a.out, len(blob)))
        return 0
    ctx = None
    if not a.host:
        import torch
        from bazuka_amd import Bzk
        torch.cuda.set_device(0)
        ctx = Bzk(0, torch.cuda.current_stream().cuda_stream)
    try:
        if a.cmd == "check":
            if (a.before is None) != (a.key is None):
                print("--before and --key come together", file=sys.stderr)
                return 2
            seed = open(a.seed_file, "rb").read(32) if a.seed_file else os.urandom(32)
            before = open(a.before, "rb").read() if a.before else None
            key = open(a.key, "rb").read() if a.key else None
            verdict, report = L.ptau_check(ctx, before, key, open(a.after, "rb").read(), seed)
            if verdict == 1:
                print("accumulator accepted" + (" as one contribution on top of %s" % a.before if a.before else ""))
                return 0
            print("accumulator REFUSED: %s[%d], code %d" % (ARRAYS[min(report[0], 6)], report[1], report[2]))
            return 1
        if a.secrets_file:
            raw = open(a.secrets_file, "rb").read(96)
            s = [int.from_bytes(raw[32 * i:32 * i + 32], "little") % pr.R_MOD for i in range(3)]
            if len(raw) != 96 or 0 in s:
                print("the secrets file must hold three 32-byte integers, none zero mod r", file=sys.stderr)
                return 2
        else:
            s = [int.from_bytes(os.urandom(64), "little") % (pr.R_MOD - 1) + 1 for _ in range(3)]  # 1 .. r - 1, the bias below 2^-256
        out, key = L.ptau_contribute(ctx, open(a.inp, "rb").read(), b"".join(pr.fr_to_mont_bytes(x) for x in s))
        with open(a.out, "wb") as f:
            f.write(out)
        with open(a.key, "wb") as f:
            f.write(key)
        print("wrote %s (%d bytes) and %s (576 bytes)" % (a.out, len(out), a.key))
        return 0
    finally:
        if ctx is not None:
            ctx.close()


if __name__ == "__main__":
    sys.exit(main())
