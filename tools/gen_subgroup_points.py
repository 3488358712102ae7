"""Writes tests/golden/subgroup_points.json: the case table of the subgroup checks (tests/subgroup_cases.py reads it).

Per group, as raw Montgomery records (G1 96 B, G2 192 B) with a kind and an `inf` flag:
  subgroup   the generator, its negative, random multiples of it
  curve      random curve points (x random, y a square root): outside the subgroup with overwhelming probability
  torsion    for every prime q of the cofactor, T of exact order q (the q-part of a random point, multiplied down), and T + S for a subgroup point S; the same for the
             whole cofactor part [r] Q of a random point
  malformed  a coordinate equal to p, a coordinate of 0xff bytes, an off-curve (x, y + 1)
  identity   flagged records (inf = 1) over zeros, over 0xff bytes and over a point outside the subgroup
The expected verdicts are NOT stored: the tests compute [r] P == identity with the oracle.  Scalars here are hundreds of bits long, so the
multiplications run in Jacobian coordinates on Python integers (oracle/pyref.py's affine ladder inverts once per step).

usage: python tools/gen_subgroup_points.py [--check]"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyref as pr  # noqa: E402
from oracle import refsetup as rs  # noqa: E402

P, R, X = pr.P_MOD, pr.R_MOD, pr.BLS_X
H1 = (X + 1) ** 2 // 3
_x = -X
H2 = (_x ** 8 - 4 * _x ** 7 + 5 * _x ** 6 - 4 * _x ** 4 + 6 * _x ** 3 - 4 * _x ** 2 - 4 * _x + 13) // 9
G1_PRIMES = (3, 11, 10177, 859267, 52437899)
G2_PRIMES = (13, 23, 2713, 11953, 262069)
OUT = os.path.join(ROOT, "tests", "golden", "subgroup_points.json")


class F1:
    zero, one = 0, 1
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)
    inv = staticmethod(lambda a: pow(a, P - 2, P))


class F2:
    zero, one = pr.F2_ZERO, pr.F2_ONE
    add, sub, mul, inv = staticmethod(pr.f2_add), staticmethod(pr.f2_sub), staticmethod(pr.f2_mul), staticmethod(pr.f2_inv)


def jdbl(F, p):
    if p is None:
        return None
    x, y, z = p
    a, b = F.mul(x, x), F.mul(y, y)
    c = F.mul(b, b)
    t = F.add(x, b)
    d = F.sub(F.sub(F.mul(t, t), a), c)
    d = F.add(d, d)
    e = F.add(F.add(a, a), a)
    x3 = F.sub(F.mul(e, e), F.add(d, d))
    c8 = F.add(c, c)
    c8 = F.add(c8, c8)
    c8 = F.add(c8, c8)
    yz = F.mul(y, z)
    return (x3, F.sub(F.mul(e, F.sub(d, x3)), c8), F.add(yz, yz))


def jadd_affine(F, p, q):
    """p Jacobian or None, q affine (never the identity)"""
    if p is None:
        return (q[0], q[1], F.one)
    x, y, z = p
    zz = F.mul(z, z)
    u2, s2 = F.mul(q[0], zz), F.mul(q[1], F.mul(z, zz))
    h, r = F.sub(u2, x), F.sub(s2, y)
    if h == F.zero:
        return jdbl(F, p) if r == F.zero else None
    hh = F.mul(h, h)
    hhh, v = F.mul(h, hh), F.mul(x, hh)
    x3 = F.sub(F.sub(F.mul(r, r), hhh), F.add(v, v))
    return (x3, F.sub(F.mul(r, F.sub(v, x3)), F.mul(y, hhh)), F.mul(z, h))


def mul(F, q, k):
    """[k] q for an affine q (or None) -> affine or None"""
    if q is None or k == 0:
        return None
    acc = None
    for bit in bin(k)[2:]:
        acc = jdbl(F, acc)
        if acc is not None and acc[2] == F.zero:
            acc = None
        if bit == "1":
            acc = jadd_affine(F, acc, q)
            if acc is not None and acc[2] == F.zero:
                acc = None
    if acc is None:
        return None
    zi = F.inv(acc[2])
    zi2 = F.mul(zi, zi)
    return (F.mul(acc[0], zi2), F.mul(acc[1], F.mul(zi, zi2)))


def add(F, p, q):
    if p is None:
        return q
    if q is None:
        return p
    r = jadd_affine(F, (p[0], p[1], F.one), q)
    if r is None or r[2] == F.zero:
        return None
    zi = F.inv(r[2])
    zi2 = F.mul(zi, zi)
    return (F.mul(r[0], zi2), F.mul(r[1], F.mul(zi, zi2)))


def random_g1(rnd):
    while True:
        x = rnd.randrange(P)
        y = rs.fp_sqrt((x ** 3 + 4) % P)
        if y is not None and y != 0:
            return (x, y if rnd.randrange(2) else P - y)


def random_g2(rnd):
    while True:
        x = (rnd.randrange(P), rnd.randrange(P))
        y = rs.fp2_sqrt(pr.f2_add(pr.f2_mul(pr.f2_sqr(x), x), pr.G2_B))
        if y is not None and y != (0, 0):
            return (x, y if rnd.randrange(2) else pr.f2_neg(y))


def is_probable_prime(n):
    if n < 2:
        return False
    for q in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def table(group, rnd):
    if group == "g1":
        F, h, primes, gen, rand, raw, size = F1, H1, G1_PRIMES, pr.G1_GEN, random_g1, pr.g1_raw96, 96
    else:
        F, h, primes, gen, rand, raw, size = F2, H2, G2_PRIMES, pr.G2_GEN, random_g2, pr.g2_raw192, 192
    order = h * R
    big = h
    for q in primes:
        assert big % q == 0, q
        while big % q == 0:
            big //= q
    if group == "g1":
        assert big == 1          # h1 = 3 * 11^2 * 10177^2 * 859267^2 * 52437899^2
    else:
        assert is_probable_prime(big) and h % 2 == 1
        primes = primes + (big,)  # the large remaining factor of h2
    rows = []
    put = lambda kind, p, inf=0: rows.append({"kind": kind, "inf": inf, "hex": (p if isinstance(p, bytes) else raw(p)).hex()})
    neg = lambda p: (p[0], F.sub(F.zero, p[1]))
    subgroup = [gen, neg(gen)] + [mul(F, gen, rnd.randrange(1, R)) for _ in range(20)]
    for p in subgroup:
        put("subgroup", p)
    curve = [rand(rnd) for _ in range(20)]
    for p in curve:
        assert mul(F, p, order) is None   # the group order is what this file says it is
        put("curve", p)
    k = 0
    for q in primes:
        rest = order   # the q-part of a random point, then down to exact order q (11^2 | h1 and E(Fp)[11] is Z_11 x Z_11: [#E / 11] kills it)
        while rest % q == 0:
            rest //= q
        while True:
            t = mul(F, rand(rnd), rest)
            if t is not None:
                break
        while mul(F, t, q) is not None:
            t = mul(F, t, q)
        assert mul(F, t, q) is None
        s = subgroup[2 + k % 20]
        k += 1
        put("torsion", t)
        put("torsion", add(F, t, s))
    while True:   # the whole cofactor part of a random point
        t = mul(F, rand(rnd), R)
        if t is not None:
            break
    put("torsion", t)
    put("torsion", add(F, t, subgroup[5]))
    # malformed records: each coordinate word in turn = p, = 0xff.., and (x, y + 1)
    good = raw(subgroup[3])
    n_coord = size // 48
    for c in range(n_coord):
        put("malformed", good[:48 * c] + P.to_bytes(48, "little") + good[48 * c + 48:])
        put("malformed", good[:48 * c] + b"\xff" * 48 + good[48 * c + 48:])
    p3 = subgroup[4]
    put("malformed", (p3[0], F.add(p3[1], F.one)))
    put("malformed", (F.add(p3[0], F.one), p3[1]))
    put("identity", bytes(size), 1)
    put("identity", b"\xff" * size, 1)
    put("identity", curve[0], 1)
    return rows


def build():
    rnd = random.Random(0x5B6)
    return {"g1": table("g1", rnd), "g2": table("g2", rnd)}


if __name__ == "__main__":
    doc = json.dumps(build(), indent=0) + "\n"
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT).read() == doc else 1)
    with open(OUT, "w") as f:
        f.write(doc)
    print("wrote", OUT)
