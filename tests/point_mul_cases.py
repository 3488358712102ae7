"""What the tests of the per-point multiplication (bzk_g1_mul_batch, bzk_g2_mul_batch, the powers forms) and of the powers-of-tau accumulator share: the
scalar table, the lane order that mixes its entries inside every wavefront, the oracle's products (computed once per size) and the accumulator's layout."""
import functools
import random

from oracle import coracle as co
from oracle import pyref as pr

R = pr.R_MOD
X2 = 0xd201000000010000 ** 2
SIZE = {"g1": 96, "g2": 192}
N_MAX = 257


def scalar_table():
    """0, 1, 2, r - 1, (r + 1) / 2; the first rounding branch of decompose2; the points where P +- X^2 P meet; the carry2 branch; 2^128 - 1, 2^128, 2^254;
    six seeded random values"""
    rnd = random.Random(20250)
    h = X2 // 2 + 1
    return [0, 1, 2, R - 1, (R + 1) // 2, X2 // 2, X2 // 2 + 1, X2 // 2 + 2, X2 - 1, X2, X2 + 1, h * X2 % R, (h * X2 + h) % R,
            2 ** 128 - 1, 2 ** 128, 2 ** 254] + [rnd.randrange(R) for _ in range(6)]


def lane_scalars(n: int):
    """lane j takes entry (7 j) mod len: 7 and the table's length are coprime, so every wave holds every entry and neighbours differ"""
    t = scalar_table()
    return [t[(7 * j) % len(t)] for j in range(n)]


def points(group: str, n: int) -> bytes:
    return (co.g1_bases if group == "g1" else co.g2_bases)(7, 0, n)


def oracle_products(group: str, pts: bytes, ks):
    """(out, inf) as the library writes them: an identity is zero bytes with its flag set"""
    sz, mul = SIZE[group], co.g1_mul if group == "g1" else co.g2_mul
    out, inf = [], []
    for i, k in enumerate(ks):
        q = mul(pts[sz * i:sz * i + sz] + b"\0", pr.fr_to_canon_bytes(k))
        inf.append(q[sz])
        out.append(bytes(sz) if q[sz] else q[:sz])
    return b"".join(out), bytes(inf)


@functools.lru_cache(maxsize=None)
def reference(group: str):
    """(points, scalars, products, flags) for N_MAX lanes of the table; every size below takes a prefix"""
    pts, ks = points(group, N_MAX), lane_scalars(N_MAX)
    out, inf = oracle_products(group, pts, ks)
    return pts, ks, out, inf


def mont(ks) -> bytes:
    return b"".join(pr.fr_to_mont_bytes(k) for k in ks)


def canon(ks) -> bytes:
    return b"".join(pr.fr_to_canon_bytes(k) for k in ks)


# ---- the accumulator: "BZKPTAU1" | u32 log_m | u32 0 | tau_g1[2m - 1] | tau_g2[m] | alpha_g1[m] | beta_g1[m] | beta_g2
ARRAYS = ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")   # report[0] - 1 of bzk_ptau_check


def layout(log_m: int):
    """{array: (offset, count, record size)} and the blob's length"""
    m = 1 << log_m
    at, out = 16, {}
    for name, cnt, sz in (("tau_g1", 2 * m - 1, 96), ("tau_g2", m, 192), ("alpha_g1", m, 96), ("beta_g1", m, 96), ("beta_g2", 1, 192)):
        out[name] = (at, cnt, sz)
        at += cnt * sz
    return out, at


def entry(blob: bytes, log_m: int, name: str, i: int) -> bytes:
    off, _, sz = layout(log_m)[0][name]
    return blob[off + sz * i:off + sz * (i + 1)]


def with_entry(blob: bytes, log_m: int, name: str, i: int, rec: bytes) -> bytes:
    off, _, sz = layout(log_m)[0][name]
    assert len(rec) == sz
    return blob[:off + sz * i] + rec + blob[off + sz * (i + 1):]


def oracle_accumulator(log_m: int, tau: int, alpha: int, beta: int) -> bytes:
    """tau^i G1, tau^i G2, alpha tau^i G1, beta tau^i G1, beta G2 by the oracle's multiplications of the generators"""
    m = 1 << log_m
    g1, g2 = co.g1_generator(), co.g2_generator()
    k = pr.fr_to_canon_bytes
    out = [b"BZKPTAU1", log_m.to_bytes(4, "little"), bytes(4)]
    out += [co.g1_mul(g1, k(pow(tau, i, R)))[:96] for i in range(2 * m - 1)]
    out += [co.g2_mul(g2, k(pow(tau, i, R)))[:192] for i in range(m)]
    out += [co.g1_mul(g1, k(alpha * pow(tau, i, R)))[:96] for i in range(m)]
    out += [co.g1_mul(g1, k(beta * pow(tau, i, R)))[:96] for i in range(m)]
    out += [co.g2_mul(g2, k(beta))[:192]]
    return b"".join(out)


def oracle_key(tau: int, alpha: int, beta: int) -> bytes:
    return b"".join(co.g2_mul(co.g2_generator(), pr.fr_to_canon_bytes(s))[:192] for s in (tau, alpha, beta))
