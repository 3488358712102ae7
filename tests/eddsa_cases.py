"""Inputs of the signature-verifier tests (tests/test_eddsa_cpu.py, tests/test_gpu_eddsa.py): the fixed case list with its expected verdicts from
oracle/pyref.py, and the seeded bulk sets.  Every entry is (pub_xy 64 bytes, msg 32, sig 96 = r.x | r.y | s), Montgomery limbs."""
import concurrent.futures
import random

from bazuka_amd import lib as L
from oracle import pyref as pr

F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
R = pr.R_MOD
ORDER = pr.JJ_ORDER
NEG1 = (0, R - 1)  # the point of order 2

CLASSES = ("valid", "msg", "s", "r.x", "pk.x", "pk.y", "other R", "other pk", "s + ORDER", "pk = (0, 1)", "pk = (0, -1)", "pk outside the subgroup",
           "non-canonical")


def entry(pk, msg, rr, s):
    return F(pk[0]) + F(pk[1]), F(msg), F(rr[0]) + F(rr[1]) + F(s)


def pyref_verdict(pk, msg, rr, s):
    return 1 if pr.jj_verify(pk, msg, (rr, s)) else 0


def signed(seed: bytes, msg: int):
    """(pk, R, s) as integers, signed by the product's host signer (checked against pyref by tests/test_host_mpn_cpu.py)"""
    key = L.host_jubjub_keys(seed)
    sig = L.host_jubjub_sign(key, F(msg))
    return (U(key[:32]), U(key[32:64])), (U(sig[:32]), U(sig[32:64])), U(sig[64:])


def order2_hits(want_other: int, want_same: int):
    """valid signatures under pk = (0, -1): s random, R = s BASE or s BASE + pk, whichever makes h pk + R == s BASE (h pk is pk for odd h, the
    identity for even h - h the full integer).  `other`: h mod ORDER has the other parity than h, so a verifier that reduces h rejects these."""
    rnd = random.Random(1)
    other, same = [], []
    while len(other) < want_other or len(same) < want_same:
        s, msg = rnd.randrange(ORDER), rnd.randrange(R)
        sb = pr.jj_mul(pr.JJ_BASE, s)
        for rr, parity in ((sb, 0), (pr.jj_add(sb, NEG1), 1)):
            h = pr.poseidon([rr[0], rr[1], NEG1[0], NEG1[1], msg])
            if h % 2 == parity:
                (other if (h % ORDER) % 2 != parity else same).append((NEG1, msg, rr, s))
                break
    return other[:want_other] + same[:want_same]


_cases = None


def case_list():
    """[(class, pub_xy, msg, sig, expected verdict)]; built once per process (about 60 pure-Python verifications)"""
    global _cases
    if _cases is not None:
        return _cases
    rnd = random.Random(20240607)
    out = []

    def add(cls, pk, msg, rr, s):
        out.append((cls,) + entry(pk, msg, rr, s) + (pyref_verdict(pk, msg, rr, s),))

    base = []
    for k in range(8):
        msg = rnd.randrange(R)
        pk, rr, s = signed(b"eddsa case %d" % k, msg)
        base.append((pk, msg, rr, s))
        add("valid", pk, msg, rr, s)
    for pk, msg, rr, s in base:  # one field changed; the last three leave the curve
        add("msg", pk, (msg + 1) % R, rr, s)
        add("s", pk, msg, rr, (s + 1) % R)
        add("r.x", pk, msg, ((rr[0] + 1) % R, rr[1]), s)
        add("pk.x", ((pk[0] + 1) % R, pk[1]), msg, rr, s)
        add("pk.y", (pk[0], (pk[1] + 1) % R), msg, rr, s)
    (pk, msg, rr, s), (pk2, _, rr2, _) = base[0], base[1]
    add("other R", pk, msg, rr2, s)
    add("other pk", pk2, msg, rr, s)
    add("s + ORDER", pk, msg, rr, s + ORDER)
    add("s + ORDER", base[2][0], base[2][1], base[2][2], base[2][3] + 7 * ORDER)
    s1 = rnd.randrange(ORDER)
    add("pk = (0, 1)", (0, 1), rnd.randrange(R), pr.jj_mul(pr.JJ_BASE, s1), s1)
    for c in order2_hits(3, 1):
        add("pk = (0, -1)", *c)
    for pk, msg, rr, s in base[3:5]:
        add("pk outside the subgroup", pr.jj_add(pk, NEG1), msg, rr, s)
    # not the limbs of a residue: neither oracle defines these; the verdict is pinned to 0
    pub, m, sig = entry(*base[5])
    for bad in (R.to_bytes(32, "little"), b"\xff" * 32):
        out.append(("non-canonical", pub, bad, sig, 0))                      # msg
        out.append(("non-canonical", pub, m, sig[:64] + bad, 0))             # s
        out.append(("non-canonical", pub, m, sig[:32] + bad + sig[64:], 0))  # r.y
        out.append(("non-canonical", bad + pub[32:], m, sig, 0))             # pk.x
    _cases = out
    return out


def bulk(n: int, seed: int):
    """n seeded entries as three byte strings: the even ones valid, the odd ones with one uniformly chosen field replaced by a random residue"""
    rnd = random.Random(seed)
    keys = [L.host_jubjub_keys(b"eddsa bulk %d %d" % (seed, k)) for k in range(16)]
    draws = [(keys[rnd.randrange(16)], F(rnd.randrange(R)), rnd.randrange(6), F(rnd.randrange(R))) for _ in range(n)]

    def make(i):
        key, msg, which, other = draws[i]
        sig = L.host_jubjub_sign(key, msg)
        fields = [key[:32], key[32:64], msg, sig[:32], sig[32:64], sig[64:]]
        if i & 1:
            fields[which] = other
        return b"".join(fields)

    with concurrent.futures.ThreadPoolExecutor(min(16, max(1, n))) as ex:
        rows = list(ex.map(make, range(n)))
    return b"".join(r[:64] for r in rows), b"".join(r[64:96] for r in rows), b"".join(r[96:] for r in rows)


def host_verdicts(pub: bytes, msg: bytes, sig: bytes, threads: int = 16) -> bytes:
    """bzk_host_jubjub_verify per entry, on a thread pool (ctypes releases the interpreter lock during the call)"""
    n = len(msg) // 32
    lib = L.load_library()

    def run(lo, hi):
        return bytes(lib.bzk_host_jubjub_verify(pub[64 * i:64 * i + 64], msg[32 * i:32 * i + 32], sig[96 * i:96 * i + 96]) for i in range(lo, hi))

    threads = max(1, min(threads, 16, n))
    step = (n + threads - 1) // threads
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        return b"".join(ex.map(lambda lo: run(lo, min(n, lo + step)), range(0, n, step)))
