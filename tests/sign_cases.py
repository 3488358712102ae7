"""Inputs of the signing tests (tests/test_eddsa_sign_cpu.py, tests/test_gpu_eddsa_sign.py): seeded distinct (key, message) rows, the crafted key
rows with their signatures by oracle/pyref.py::jj_sign, rows with a field that is not a residue's limbs, seeds at the SHA3 rate boundary, and
transaction records with their keys.  Keys are 128 bytes pub.x | pub.y | randomness | scalar, scalars 32-byte Montgomery limbs.  Expected values
are computed once per process and never changed."""
import random

import decompress_cases as D
from bazuka_amd import lib as L
from oracle import pyref as pr

F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
R, ORDER = pr.R_MOD, pr.JJ_ORDER
SEED_LENGTHS = (0, 1, 135, 136, 137, 300)  # the SHA3 rate is 136 bytes: one block with room, exactly full (a second block of padding), two blocks
FIELDS = ("pub.x", "pub.y", "randomness", "scalar", "msg")

_keys = {}


def key_of(seed: bytes) -> bytes:
    if seed not in _keys:
        _keys[seed] = L.host_jubjub_keys(seed)
    return _keys[seed]


def key_bytes(sk) -> bytes:
    return F(sk["pub"][0]) + F(sk["pub"][1]) + F(sk["randomness"]) + F(sk["scalar"])


def key_dict(key: bytes):
    return {"pub": (U(key[:32]), U(key[32:64])), "randomness": U(key[64:96]), "scalar": U(key[96:128])}


def sig_bytes(sig) -> bytes:
    (rx, ry), s = sig
    return F(rx) + F(ry) + F(s)


def rows(n: int, seed: int):
    """n distinct (key, message) rows over 64 keys: (keys n x 128, msgs n x 32)"""
    rnd = random.Random(seed)
    keys = [key_of(b"sign case %d" % k) for k in range(min(n, 64))]
    msgs = set()
    while len(msgs) < n:
        msgs.add(rnd.randrange(R))
    return b"".join(keys[i % len(keys)] for i in range(n)), b"".join(F(m) for m in sorted(msgs))


_crafted = None


def crafted():
    """[(class, key bytes, msg bytes, signature bytes by pyref.jj_sign)]: the key is caller bytes, so scalar and randomness are free"""
    global _crafted
    if _crafted is not None:
        return _crafted
    base, other = key_dict(key_of(b"sign crafted")), key_dict(key_of(b"sign crafted other"))
    cases = []
    for a in (0, 1, ORDER - 1, ORDER, R - 1):
        cases.append(("scalar %d" % a if a < 2 else "scalar %s" % {ORDER - 1: "ORDER - 1", ORDER: "ORDER", R - 1: "R_MOD - 1"}[a],
                      dict(base, scalar=a), 123456))
    for b in (0, R - 1):
        cases.append(("randomness %s" % ("0" if b == 0 else "R_MOD - 1"), dict(base, randomness=b), 123456))
    for m in (0, R - 1):
        cases.append(("msg %s" % ("0" if m == 0 else "R_MOD - 1"), base, m))
    cases.append(("pub of another key", dict(base, pub=other["pub"]), 123456))
    cases.append(("everything at the top", dict(base, randomness=R - 1, scalar=R - 1), R - 1))
    _crafted = [(w, key_bytes(sk), F(m), sig_bytes(pr.jj_sign(sk, m))) for w, sk, m in cases]
    return _crafted


def non_residue_rows():
    """[(field, key bytes, msg bytes)]: one field in turn holds the modulus' own limbs, then 2^256 - 1"""
    key, msg = key_of(b"sign non-residue"), F(424242)
    out = []
    for bad in (D.R_LIMBS, D.ALL_ONES):
        for f in range(4):
            out.append((FIELDS[f], key[:32 * f] + bad + key[32 * f + 32:], msg))
        out.append((FIELDS[4], key, bad))
    return out


def interleaved(n: int, seed: int):
    """n distinct rows with the crafted and the non-residue rows, alternating, spread among them (a wavefront of 64 that holds several holds both
    kinds): (keys, msgs, want ok bytes, {row: expected signature bytes} for the crafted rows)"""
    keys, msgs = rows(n, seed)
    good, bad = [(c[1], c[2], 1, c[3]) for c in crafted()], [(b[1], b[2], 0, None) for b in non_residue_rows()]
    special = [r for pair in zip(good, bad) for r in pair] + good[len(bad):] + bad[len(good):]
    step = max(1, n // len(special))
    out = []
    for i in range(n):
        out.append((keys[128 * i:128 * i + 128], msgs[32 * i:32 * i + 32], 1, None))
        if i % step == step - 1 and special:
            out.append(special.pop(0))
    out += special
    return (b"".join(r[0] for r in out), b"".join(r[1] for r in out), bytes(r[2] for r in out),
            {i: r[3] for i, r in enumerate(out) if r[3] is not None})


def seeds(n: int = len(SEED_LENGTHS)):
    """n seeded seeds whose lengths cycle through SEED_LENGTHS"""
    rnd = random.Random(77)
    return [bytes(rnd.randrange(256) for _ in range(SEED_LENGTHS[i % len(SEED_LENGTHS)])) for i in range(n)]


def tx_records(n: int, seed: int, spoil_every: int = 0):
    """n unsigned transaction records over the token-pair forms (190, 222 and 254 bytes) with their keys: (keys n x 128, [dict], spoiled rows).
    Every spoil_every-th record has, in turn, a dst.x without a root or a flipped src oddity."""
    rnd = random.Random(seed)
    dsts = [D.compress(key_of(b"sign tx dst %d" % k)[:64]) for k in range(16)]
    keys, txs, spoiled = [], [], []
    for i in range(n):
        key = key_of(b"sign tx src %d" % (i % 32))
        a, f = D.TOKEN_PAIRS[i % len(D.TOKEN_PAIRS)]
        t = dict(nonce=1 + i, src=D.compress(key[:64]), dst=dsts[rnd.randrange(16)], atok=a, amount=10 ** 6 + i, ftok=f, fee=i % 7, sig=bytes(96))
        if spoil_every and i % spoil_every == spoil_every - 1:
            t = D.mutate(t, "dst.x without a root" if len(spoiled) % 2 == 0 else "src oddity", rnd)
            spoiled.append(i)
        keys.append(key)
        txs.append(t)
    return b"".join(keys), txs, spoiled
