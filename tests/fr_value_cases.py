"""Structured and top-of-range Fr inputs, as RAW Montgomery limb integers (what raw_fr_bytes below writes unchanged).

rand_scalars_bytes clears the top two bits, so its raw values stay below 2^254 while r is about 2^254.86: 45 % of the field - the part
with the largest top 29-bit limb - is never an input, and residue 0 (whose products come out as exactly r, not 0) almost never an
operand.  These patterns are both: every function of n returns n integers below r, seeded, the same on every machine."""
import functools
import random

from util import pr

FR_MONT_R, R_MOD, SEED = pr.FR_MONT_R, pr.R_MOD, pr.SEED

RM1 = R_MOD - 1
LIMB_K = tuple(range(29, 233, 29)) + (254,)     # 29, 58, .., 232: the limb boundaries of the 9 x 29-bit form ; 254: the top of the old inputs
LIMB_VALUES = tuple(v for k in LIMB_K for v in ((1 << k) - 1, 1 << k, R_MOD - (1 << k)))


def raw_fr_bytes(ints):
    """each integer below r as 32 little-endian bytes: the RAW Montgomery limbs themselves, no conversion applied (what util.rand_scalars_bytes never
    produces above 2^254)"""
    out = bytearray()
    for v in ints:
        assert 0 <= v < R_MOD, hex(v)
        out += v.to_bytes(32, "little")
    return bytes(out)


def _checked(vals, n):
    assert len(vals) == n and all(0 <= v < R_MOD for v in vals)
    return vals


def zeros(n):
    return _checked([0] * n, n)


def const_rm1(n):
    return _checked([RM1] * n, n)


def const_one(n):
    """every value the Montgomery form of 1"""
    return _checked([FR_MONT_R] * n, n)


def delta(n, j):
    """raw r - 1 at j, 0 elsewhere"""
    v = [0] * n
    v[j] = RM1
    return _checked(v, n)


def delta_positions(n):
    return sorted({0, 1 % n, n // 2, n - 1})


def alt(n):
    return _checked([RM1 if i & 1 else 0 for i in range(n)], n)


@functools.lru_cache(maxsize=None)
def _top(n, seed):
    rng = random.Random((seed << 8) ^ n)
    return tuple(rng.randrange(1 << 254, R_MOD) for _ in range(n))


def top(n, seed=SEED):
    """uniform raw values in [2^254, r)"""
    return _checked(list(_top(n, seed)), n)


def limbs(n):
    """2^k - 1, 2^k and r - 2^k for k at the 29-bit limb boundaries and 254, cycled: all-ones and all-zero limbs next to each other"""
    return _checked([LIMB_VALUES[i % len(LIMB_VALUES)] for i in range(n)], n)


def sparse(n, seed=SEED):
    """`top` with 15 of every 16 elements zeroed"""
    return _checked([v if i % 16 == 0 else 0 for i, v in enumerate(_top(n, seed))], n)


def uniform(n, seed=SEED):
    """uniform raw values in [0, r): the CPU replay's extra pattern"""
    rng = random.Random((seed << 8) ^ n ^ 0x55)
    return _checked([rng.randrange(R_MOD) for _ in range(n)], n)


LARGE = ("zeros", "top", "sparse", "delta(n-1)")   # the patterns of the sizes from 2^19 on (named(n, LARGE))
_MONT_INV =pow(FR_MONT_R, -1, R_MOD)


def raw_product(a, b):
    """raw limbs of the pointwise product: (A 2^256)(B 2^256) 2^-256"""
    return [x * y % R_MOD * _MONT_INV % R_MOD for x, y in zip(a, b)]


def h_cases(m):
    """[(name, a, b, c, expect_zero)] for the h chain at domain size m: a, b, c are the evaluation vectors (n_rows = their length, the rest of the domain is
    padding); expect_zero where A B - C is the zero polynomial, so that every coefficient of h is 0"""
    ta, tb, tc = top(m, SEED + 1), top(m, SEED + 2), top(m, SEED + 3)
    rm1 = const_rm1(m)
    return [
        ("zeros", zeros(m), zeros(m), zeros(m), True),
        ("top", ta, tb, tc, False),
        ("const_rm1 satisfied", rm1, rm1, raw_product(rm1, rm1), True),
        # a real proof's case: A B - C vanishes ON the domain (h is the non-zero quotient by Z)
        ("top satisfied", ta, tb, raw_product(ta, tb), False),
        ("top c=0", ta, tb, zeros(m), False),
        ("one row", ta[:1], tb[:1], tc[:1], False),
    ]


def named(n, which=None):
    """[(name, values)] of every pattern at size n (or of the named ones); delta(j) once per distinct position"""
    out = [("zeros", zeros), ("const_rm1", const_rm1), ("const_one", const_one)]
    out += [("delta(%d)" % j, functools.partial(delta, j=j)) for j in delta_positions(n)]
    out += [("alt", alt), ("top", top), ("limbs", limbs), ("sparse", sparse)]
    if which is not None:
        which = ["delta(%d)" % (n - 1) if w == "delta(n-1)" else w for w in which]
        missing = set(which) - {k for k, _ in out}
        assert not missing, missing
        out = [(k, f) for k, f in out if k in which]
    return [(k, f(n)) for k, f in out]
