"""Inputs of the key-decompression and transaction-admission tests (tests/test_decompress_cpu.py, tests/test_gpu_decompress.py): the fixed list of
compressed keys, a Python encoder of bincode(MpnTransaction), the transaction list with its mutations, and seeded bulk sets.  Expected values come from
oracle/pyref.py (poseidon, jj_verify, jj_on_curve) and oracle/pycircuit.py (pt_decompress) alone; scalars are 32-byte Montgomery limbs."""
import concurrent.futures
import random
import struct

import r1cs_scenarios as sc
from bazuka_amd import lib as L
from oracle import pycircuit as pc
from oracle import pyref as pr

F, U = pr.fr_to_mont_bytes, pr.fr_from_mont_bytes
R = pr.R_MOD
R_LIMBS, ALL_ONES = R.to_bytes(32, "little"), b"\xff" * 32
ZERO64 = bytes(64)


def radicand(x: int) -> int:
    x2 = x * x % R
    return (1 + x2) * pr.inv_mod((1 - pr.JJ_D * x2) % R, R) % R


def is_square(a: int) -> bool:
    """Euler's criterion; 0 counts as a square (its root is 0)"""
    return a % R == 0 or pow(a, (R - 1) // 2, R) == 1


def oracle_decompress(xb: bytes, odd):
    """(x, y) as integers from oracle/pycircuit.py, or None where the reference panics (the radicand is no square) or xb is not a residue's limbs"""
    if int.from_bytes(xb, "little") >= R:
        return None
    x = U(xb)
    if not is_square(radicand(x)):
        return None
    return pc.pt_decompress(x, bool(odd))


def expect(xb: bytes, odd):
    """(xy bytes, verdict) the product must give"""
    p = oracle_decompress(xb, odd)
    return (F(p[0]) + F(p[1]), 1) if p else (ZERO64, 0)


def compress(pub_xy: bytes):
    """PointAffine::compress: x and the parity of the canonical y"""
    return pub_xy[:32], U(pub_xy[32:64]) & 1


def fixed_keys():
    """[(class, x bytes, odd)]"""
    out = []
    for k in range(8):
        x, _ = compress(L.host_jubjub_keys(b"decompress case %d" % k))
        out += [("key", x, 0), ("key", x, 1)]
    out += [("x = 0", F(0), 0), ("x = 0", F(0), 1)]
    i = pc._sqrt_fr(R - 1)
    out += [("x^2 = -1", F(i), 0), ("x^2 = -1", F(i), 1), ("x^2 = -1", F(R - i), 0), ("x^2 = -1", F(R - i), 1)]
    rnd, found = random.Random(20240611), 0
    while found < 8:
        x = rnd.randrange(R)
        if not is_square(radicand(x)):
            out += [("no root", F(x), 0), ("no root", F(x), 1)]
            found += 1
    out += [("limbs of r", R_LIMBS, 0), ("limbs of r", R_LIMBS, 1), ("ff..ff", ALL_ONES, 0), ("ff..ff", ALL_ONES, 1)]
    return out


def bulk_keys(n: int, seed: int):
    """n seeded x (random residues: about half decompress) and oddities, as two byte strings"""
    rnd = random.Random(seed)
    return b"".join(F(rnd.randrange(R)) for _ in range(n)), bytes(rnd.randrange(2) for _ in range(n))


def host_decompress_all(x: bytes, odd: bytes, threads: int = 16):
    """bzk_host_jubjub_decompress per entry on a thread pool: (xy, ok) in the layouts of bzk_jubjub_decompress_batch"""
    n = len(odd)

    def run(lo):
        xy, ok = [], bytearray()
        for i in range(lo, min(n, lo + step)):
            p = L.host_jubjub_decompress(x[32 * i:32 * i + 32], odd[i])
            xy.append(p or ZERO64)
            ok.append(1 if p else 0)
        return b"".join(xy), bytes(ok)

    threads = max(1, min(threads, n))
    step = (n + threads - 1) // threads
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(run, range(0, n, step)))
    return b"".join(p[0] for p in parts), b"".join(p[1] for p in parts)


# ---- bincode(MpnTransaction): nonce u32 | src PointCompressed | dst PointCompressed | amount Money | fee Money | Signature
# a transaction here: dict(nonce, src=(x bytes, odd), dst=(x bytes, odd), atok, amount, ftok, fee, sig=96 bytes); token ids are integers
def enc_contract_id(tok: int) -> bytes:
    if tok == 0:
        return struct.pack("<I", 0)
    if tok == 1:
        return struct.pack("<I", 1)
    return struct.pack("<I", 2) + F(tok)


def enc_tx(t) -> bytes:
    return (struct.pack("<I", t["nonce"]) + t["src"][0] + bytes([t["src"][1]]) + t["dst"][0] + bytes([t["dst"][1]])
            + enc_contract_id(t["atok"]) + struct.pack("<Q", t["amount"]) + enc_contract_id(t["ftok"]) + struct.pack("<Q", t["fee"]) + t["sig"])


def tx_message(t, hasher=pr.poseidon):
    """tx.hash() over the decompressed dst, or None where dst does not decompress"""
    dst = oracle_decompress(*t["dst"])
    if dst is None:
        return None
    return hasher([t["nonce"], dst[0], dst[1], t["atok"], t["amount"], t["ftok"], t["fee"]])


def oracle_tx(t):
    """(verdict, hash bytes) by the pure-Python composition decompress -> poseidon -> jj_verify"""
    msg = tx_message(t)
    if msg is None:
        return 0, bytes(32)
    src = oracle_decompress(*t["src"])
    sig = t["sig"]
    ok = src is not None and pr.jj_verify(src, msg, ((U(sig[:32]), U(sig[32:64])), U(sig[64:])))
    return (1 if ok else 0), F(msg)


def _host_hash(vals):
    return U(L.host_poseidon(b"".join(F(v) for v in vals)))


def signed_tx(src_seed: bytes, dst_seed: bytes, nonce, atok, amount, ftok, fee, hasher=pr.poseidon):
    key = L.host_jubjub_keys(src_seed)
    t = dict(nonce=nonce, src=compress(key[:64]), dst=compress(L.host_jubjub_keys(dst_seed)[:64]), atok=atok, amount=amount, ftok=ftok, fee=fee)
    t["sig"] = L.host_jubjub_sign(key, F(tx_message(t, hasher)))
    return t


MUTATIONS = ("src oddity", "dst oddity", "dst.x without a root", "nonce + 1", "amount + 1", "swapped tokens", "bad s", "bad R")


def no_root_x(rnd) -> bytes:
    while True:
        x = rnd.randrange(R)
        if not is_square(radicand(x)):
            return F(x)


def mutate(t, which: str, rnd):
    m = dict(t)
    if which == "src oddity":
        m["src"] = (t["src"][0], t["src"][1] ^ 1)
    elif which == "dst oddity":
        m["dst"] = (t["dst"][0], t["dst"][1] ^ 1)
    elif which == "dst.x without a root":
        m["dst"] = (no_root_x(rnd), t["dst"][1])
    elif which == "nonce + 1":
        m["nonce"] = t["nonce"] + 1
    elif which == "amount + 1":
        m["amount"] = t["amount"] + 1
    elif which == "swapped tokens":
        m["atok"], m["ftok"] = t["ftok"], t["atok"]
    elif which == "bad s":
        m["sig"] = t["sig"][:64] + F((U(t["sig"][64:]) + 1) % R)
    elif which == "bad R":
        m["sig"] = F((U(t["sig"][:32]) + 1) % R) + t["sig"][32:]
    else:
        raise KeyError(which)
    return m


TOKEN_PAIRS = ((4242, 1), (1, 777), (4242, 777), (0, 1), (1, 1), (4242, 4242), (1, 1), (99, 1))  # Ziesha = 1, Null = 0, the rest Custom

_txs = None


def tx_list():
    """[(class, transaction, expected verdict, expected hash)]: eight signed transactions over the token-id forms (records of 190, 222 and 254 bytes),
    and every mutation of four of them; expectations from oracle_tx.  Built once per process."""
    global _txs
    if _txs is not None:
        return _txs
    rnd = random.Random(20240612)
    base = [signed_tx(b"tx src %d" % k, b"tx dst %d" % k, 1 + k, a, 1000 + 17 * k, f, k % 5) for k, (a, f) in enumerate(TOKEN_PAIRS)]
    out = [("valid", t) + oracle_tx(t) for t in base]
    for t in base[:4]:
        out += [(w, m) + oracle_tx(m) for w in MUTATIONS for m in (mutate(t, w, rnd),)]
    _txs = out
    return out


def tx_bulk(n: int, seed: int, pool: int = 192):
    """n seeded records as dicts: drawn from `pool` transactions signed over bzk_host_poseidon (the product's host hash, pinned on pyref by
    tests/test_host_mpn_cpu.py), token forms mixed so that both a short and a long record length occur; every third record carries a mutation"""
    rnd = random.Random(seed)

    def make(k):
        a, f = TOKEN_PAIRS[k % len(TOKEN_PAIRS)]
        return signed_tx(b"bulk %d src %d" % (seed, k % 24), b"bulk %d dst %d" % (seed, k % 17), 1 + k, a, 10 ** 6 + k, f, k % 7, _host_hash)

    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        signed = list(ex.map(make, range(pool)))
    out = []
    for i in range(n):
        t = signed[rnd.randrange(pool)]
        out.append(mutate(t, MUTATIONS[rnd.randrange(len(MUTATIONS))], rnd) if i % 3 == 2 else t)
    return out


# ---- admission: a world fed wire-form transactions against a twin fed through bzk_mpn_push_tx
ZIESHA = F(1)
N_ACC = 8
TRANSFERS = [(0, 1, 100, 1), (1, 2, 50, 0), (2, 3, 7, 2), (0, 4, 30, 1), (5, 0, 900, 3), (3, 3, 5, 1), (0, 9, 77, 0), (9, 6, 10, 1), (4, 5, 1, 0)]


def admission_world(dev=None):
    w = L.MpnWorld(3, 3)
    if dev is not None:
        w.set_device(dev)
    for i in range(N_ACC):
        w.add_account(i, b"acct%d" % i, ZIESHA, 10 ** 9)
    w.add_key(9, b"newcomer")
    w.set_height(5)
    return w


def _seed(i):
    return b"newcomer" if i == 9 else b"acct%d" % i


def wire_transfers():
    """TRANSFERS signed outside any world, with the nonces bzk_mpn_push_tx would assign (every account starts at nonce 0)"""
    sent, out = {}, []
    for s, d, amount, fee in TRANSFERS:
        sent[s] = sent.get(s, 0) + 1
        out.append(signed_tx(_seed(s), _seed(d), sent[s], 1, amount, 1, fee, _host_hash))
    return out


def bad_transfers(good):
    rnd = random.Random(3)
    return [mutate(good[1], "bad s", rnd), mutate(good[4], "src oddity", rnd), mutate(good[6], "amount + 1", rnd)]


def twin_work():
    twin = admission_world()
    for s, d, amount, fee in TRANSFERS:
        twin.push_tx(s, d, ZIESHA, amount, ZIESHA, fee)
    return twin.make_work(2, sc.VKS, 10, log4_batches=(1, 1, 2)), twin.root()


def admit(world, txs):
    return world.push_txs(b"".join(enc_tx(t) for t in txs), len(txs))
