// Ed25519 verification as `ed25519-dalek = "1"` `PublicKey::verify` does it (the reference's src/crypto/ed25519.rs:81-83), one signature per lane
// (eddsa.hip ed25519_verify_kernel; the CPU harness tests/host/ed25519_check.hip and the ctx = NULL entries run the same code).
//
// The crate is not vendored, so its rules are restated [recalled]:
//   - cofactorless: the verdict is encode([s]B - [k]A) == R as 32 bytes, k = SHA-512(R | A | M) mod l; no small-order rejection for A or R
//   - s >= l is refused
//   - A: bit 255 is the sign of x, the low 255 bits are y taken mod p without a canonicity check; A fails only when the radicand has no root;
//     the root is made non-negative and then negated where the sign bit is set, so x = 0 with the sign bit set is accepted
//   - the hash absorbs A's and R's bytes as given; R is never decoded, so a non-canonical R can never verify
//
// Field 2^255 - 19: ten limbs of 26 / 25 bits alternating (radix 2^25.5), unsigned, every value kept carried (even limbs < 2^26 + 2^20, odd limbs
// < 2^25 + 2^20).  A product is 100 32 x 32 -> 64 multiply-adds (v_mad_u64_u32) into ten columns: the terms that wrap past 2^255 use 19 b_j
// (32 bits), the odd-odd terms 2 a_i, so the columns need no fold afterwards - one carry chain ends the product.  No Montgomery form.
//
// Group: extended coordinates on -x^2 + y^2 = 1 + d x^2 y^2.  [k](-A) runs on signed 3-bit windows (85 digits in [-4, 4), three doublings and
// one addition each) against the lane's own table {1, 2, 3, 4}(-A) in LDS, one column per lane; [s]B adds 64 entries of a per-context table of
// j 16^i B (global memory, built once) with no doublings.  Every lane runs the same instructions: a digit selects a table index and a sign, the
// scalars' words sit in the lane's LDS column and nothing per lane is indexed in registers.
#pragma once
#include <vector>

#include "bzk_sha512.cuh"

#if defined(BZK_FP28_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
#include <assert.h>
#define BZK_ED_ASSERT(x) assert(x)
#else
#define BZK_ED_ASSERT(x)
#endif

namespace bzk {
namespace ed25519 {

struct Fe {
    uint32_t l[10];
};
constexpr uint32_t M26 = (1u << 26) - 1, M25 = (1u << 25) - 1;
BZK_HD constexpr int limb_bits(int i) { return (i & 1) ? 25 : 26; }
BZK_HD constexpr uint32_t limb_mask(int i) { return (i & 1) ? M25 : M26; }
BZK_HD constexpr int limb_off(int i) { return (51 * i + 1) / 2; }  // 0, 26, 51, 77, 102, 128, 153, 179, 204, 230

static constexpr uint32_t FE_D[10] = {0x35978a3, 0x0d37284, 0x3156ebd, 0x06a0a0e, 0x001c029, 0x179e898, 0x3a03cbb, 0x1ce7198, 0x2e2b6ff, 0x1480db3};
static constexpr uint32_t FE_D2[10] = {0x2b2f159, 0x1a6e509, 0x22add7a, 0x0d4141d, 0x0038052, 0x0f3d130, 0x3407977, 0x19ce331, 0x1c56dff, 0x0901b67};
static constexpr uint32_t FE_SQRTM1[10] = {0x20ea0b0, 0x186c9d2, 0x08f189d, 0x035697f, 0x0bd0c60,
                                           0x1fbd7a7, 0x2804c9e, 0x1e16569, 0x004fc1d, 0x0ae0c92};

BZK_HD void fe_check(const Fe& a) {
#pragma unroll
    for (int i = 0; i < 10; ++i) BZK_ED_ASSERT(a.l[i] < (1u << limb_bits(i)) + (1u << 20));
    (void)a;
}
BZK_HD Fe fe_const(const uint32_t (&c)[10]) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.l[i] = c[i];
    return r;
}
BZK_HD Fe fe_small(uint32_t v) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.l[i] = i ? 0 : v;
    return r;
}
BZK_HD Fe fe_sel(bool c, const Fe& a, const Fe& b) {  // c ? a : b
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
// limbs below 2^31 in, carried out
BZK_HD Fe fe_carry(Fe a) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        a.l[i + 1] += a.l[i] >> limb_bits(i);
        a.l[i] &= limb_mask(i);
    }
    a.l[0] += 19 * (a.l[9] >> 25);
    a.l[9] &= M25;
    return a;
}
BZK_HD Fe fe_add(const Fe& a, const Fe& b) {
    fe_check(a); fe_check(b);
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.l[i] = a.l[i] + b.l[i];
    return fe_carry(r);
}
BZK_HD Fe fe_sub(const Fe& a, const Fe& b) {  // a + 4 p - b
    fe_check(a); fe_check(b);
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.l[i] = a.l[i] + (i == 0 ? (1u << 28) - 76 : (i & 1) ? (1u << 27) - 4 : (1u << 28) - 4) - b.l[i];
    return fe_carry(r);
}
BZK_HD Fe fe_neg(const Fe& a) { return fe_sub(fe_small(0), a); }

// the term a_i b_j belongs to column (i + j) mod 10, times 19 where i + j >= 10, times 2 where i and j are both odd
BZK_HD Fe fe_mul(const Fe& a, const Fe& b) {
    fe_check(a); fe_check(b);
    uint32_t b19[10], a2[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        b19[i] = 19 * b.l[i];
        a2[i] = (i & 1) ? 2 * a.l[i] : a.l[i];
    }
    uint64_t z[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) z[k] = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const uint32_t x = (j & 1) ? a2[i] : a.l[i];
            const uint32_t y = i + j >= 10 ? b19[j] : b.l[j];
            BZK_ED_ASSERT(z[(i + j) % 10] + (uint64_t)x * y >= z[(i + j) % 10]);  // host harness: the column must not wrap
            z[(i + j) % 10] += (uint64_t)x * y;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        z[i + 1] += z[i] >> limb_bits(i);
        z[i] &= limb_mask(i);
    }
    z[0] += 19 * (z[9] >> 25);
    z[9] &= M25;
    z[1] += z[0] >> 26;
    z[0] &= M26;
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.l[i] = (uint32_t)z[i];
    fe_check(r);
    return r;
}
// a square: the 45 off-diagonal terms are taken once against a doubled operand, 55 multiply-adds
BZK_HD Fe fe_sq(const Fe& a) {
    fe_check(a);
    uint32_t a19[10], a2[10], a4[10];  // a4: 2 x the doubled odd limb (an odd-odd off-diagonal term is doubled twice)
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        a19[i] = 19 * a.l[i];
        a2[i] = 2 * a.l[i];
        a4[i] = 4 * a.l[i];
    }
    uint64_t z[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) z[k] = 0;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
#pragma unroll
        for (int j = i; j < 10; ++j) {
            const bool oo = (i & 1) && (j & 1);
            const uint32_t x = i == j ? (oo ? a2[i] : a.l[i]) : (oo ? a4[i] : a2[i]);
            const uint32_t y = i + j >= 10 ? a19[j] : a.l[j];
            BZK_ED_ASSERT(z[(i + j) % 10] + (uint64_t)x * y >= z[(i + j) % 10]);
            z[(i + j) % 10] += (uint64_t)x * y;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        z[i + 1] += z[i] >> limb_bits(i);
        z[i] &= limb_mask(i);
    }
    z[0] += 19 * (z[9] >> 25);
    z[9] &= M25;
    z[1] += z[0] >> 26;
    z[0] &= M26;
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.l[i] = (uint32_t)z[i];
    fe_check(r);
    return r;
}
BZK_HD Fe fe_sqn(Fe a, int n) {
#pragma unroll 1
    for (int i = 0; i < n; ++i) a = fe_sq(a);
    return a;
}
// z^(2^252 - 3) = z^((p - 5) / 8)
BZK_HD Fe fe_pow22523(const Fe& z) {
    Fe t0 = fe_sq(z);                      // 2
    Fe t1 = fe_mul(z, fe_sqn(t0, 2));      // 9
    t0 = fe_mul(t0, t1);                   // 11
    t0 = fe_mul(t1, fe_sq(t0));            // 31 = 2^5 - 1
    t0 = fe_mul(fe_sqn(t0, 5), t0);        // 2^10 - 1
    t1 = fe_mul(fe_sqn(t0, 10), t0);       // 2^20 - 1
    t1 = fe_mul(fe_sqn(t1, 20), t1);       // 2^40 - 1
    t0 = fe_mul(fe_sqn(t1, 10), t0);       // 2^50 - 1
    t1 = fe_mul(fe_sqn(t0, 50), t0);       // 2^100 - 1
    t1 = fe_mul(fe_sqn(t1, 100), t1);      // 2^200 - 1
    t0 = fe_mul(fe_sqn(t1, 50), t0);       // 2^250 - 1
    return fe_mul(fe_sqn(t0, 2), z);       // 2^252 - 3
}
// z^(p - 2): 8 (2^252 - 3) + 3 = 2^255 - 21
BZK_HD Fe fe_invert(const Fe& z) { return fe_mul(fe_sqn(fe_pow22523(z), 3), fe_mul(fe_sq(z), z)); }

// the low 255 bits of 32 little-endian bytes (8 words) as limbs: a value below 2^255, not reduced
BZK_HD Fe fe_from_words(const uint32_t (&w)[8]) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const int off = limb_off(i), k = off >> 5, sh = off & 31;
        const uint64_t v = (uint64_t)w[k] | (k + 1 < 8 ? (uint64_t)w[k + 1] << 32 : 0);
        r.l[i] = (uint32_t)(v >> sh) & limb_mask(i);
    }
    return r;
}
// the canonical residue's 32 little-endian bytes as 8 words (bit 255 clear)
BZK_HD void fe_to_words(const Fe& a, uint32_t (&w)[8]) {
    fe_check(a);
    uint32_t q = 19;  // the carry out of bit 255 of a + 19: 1 exactly where a >= p (a < 2 p)
#pragma unroll
    for (int i = 0; i < 10; ++i) q = (a.l[i] + q) >> limb_bits(i);
    uint32_t t[10], c = 19 * q;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t v = a.l[i] + c;
        t[i] = v & limb_mask(i);
        c = v >> limb_bits(i);
    }
    uint64_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const int off = limb_off(i), k = off >> 6, sh = off & 63;
        o[k] |= (uint64_t)t[i] << sh;
        if (sh + limb_bits(i) > 64) o[k + 1] |= (uint64_t)t[i] >> (64 - sh);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[2 * i] = (uint32_t)o[i];
        w[2 * i + 1] = (uint32_t)(o[i] >> 32);
    }
}
BZK_HD bool fe_is_zero(const Fe& a) {
    uint32_t w[8], any = 0;
    fe_to_words(a, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) any |= w[i];
    return any == 0;
}
BZK_HD bool fe_is_negative(const Fe& a) {
    uint32_t w[8];
    fe_to_words(a, w);
    return (w[0] & 1) != 0;
}

// ---- scalars mod l = 2^252 + c ------------------------------------------------------------------------------------
static constexpr uint32_t SC_C[4] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu};
static constexpr uint32_t SC_L[8] = {0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0, 0, 0, 0x10000000u};
static constexpr uint32_t SC_2L[8] = {0xb9eba7dau, 0xb024c634u, 0x45ef39acu, 0x29bdf3bdu, 0, 0, 0, 0x20000000u};

template <int N>
BZK_HD void sc_mul_c(const uint32_t (&a)[N], uint32_t (&out)[N + 4]) {
#pragma unroll
    for (int i = 0; i < N + 4; ++i) out[i] = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t v = (uint64_t)a[i] * SC_C[j] + out[i + j] + carry;
            out[i + j] = (uint32_t)v;
            carry = v >> 32;
        }
        out[i + 4] = (uint32_t)carry;
    }
}
// x = hi 2^252 + lo
template <int N>
BZK_HD void sc_split(const uint32_t (&x)[N], uint32_t (&lo)[8], uint32_t (&hi)[N - 7]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) lo[i] = i == 7 ? x[7] & 0x0fffffffu : x[i];
#pragma unroll
    for (int i = 0; i < N - 7; ++i) hi[i] = (x[7 + i] >> 28) | (8 + i < N ? x[8 + i] << 4 : 0);
}
BZK_HD bool sc_below_l(const uint32_t (&s)[8]) {
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) borrow = (((uint64_t)s[i] - SC_L[i] - borrow) >> 63) & 1;
    return borrow != 0;
}
// the 64-byte digest as a little-endian integer, mod l.  2^252 = -c (mod l) three times over: x = lo - hi c, hi c = tlo - thi c,
// thi c = ulo - uhi c, so x = lo - tlo + ulo - uhi c, every term below 2^252 + 2^133; 2 l is added to keep it positive and at most three
// subtractions of l (selects) remain
BZK_HD void sc_reduce512(const uint32_t (&x)[16], uint32_t (&out)[8]) {
    uint32_t lo[8], hi[9], t[13], tlo[8], thi[6], u[10], ulo[8], uhi[3], v[7];
    sc_split<16>(x, lo, hi);
    sc_mul_c<9>(hi, t);
    sc_split<13>(t, tlo, thi);
    sc_mul_c<6>(thi, u);
    sc_split<10>(u, ulo, uhi);
    sc_mul_c<3>(uhi, v);
    int64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t a = (int64_t)lo[i] + ulo[i] + SC_2L[i] - tlo[i] - (i < 7 ? v[i] : 0) + carry;
        out[i] = (uint32_t)a;
        carry = a >> 32;
    }
    BZK_ED_ASSERT(carry == 0);
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        uint32_t d[8];
        uint64_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t y = (uint64_t)out[i] - SC_L[i] - borrow;
            d[i] = (uint32_t)y;
            borrow = (y >> 63) & 1;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = borrow ? out[i] : d[i];
    }
    BZK_ED_ASSERT(sc_below_l(out));
}

// ---- the group ----------------------------------------------------------------------------------------------------
struct Pt {
    Fe X, Y, Z, T;  // x = X / Z, y = Y / Z, x y = T / Z
};
struct Cached {
    Fe YpX, YmX, Z, T2d;
};
constexpr int CACHED_WORDS = 40, NIELS_WORDS = 30;
constexpr int VAR_TAB = 4;                                      // {1, 2, 3, 4}(-A)
constexpr int VAR_DIGITS = 85;                                  // signed 3-bit digits of a scalar below 2^253
constexpr int LANE_WORDS = VAR_TAB * CACHED_WORDS + 9 + 8;      // the table, k + bias (and a zero word above it), s: 708 bytes per lane
constexpr int BASE_WINDOWS = 64, BASE_ENTRIES = 16;             // j 16^i B, j = 0 .. 15 (entry 0: the neutral element)
constexpr size_t BASE_TAB_WORDS = (size_t)BASE_WINDOWS * BASE_ENTRIES * NIELS_WORDS;  // 120 KB
// 4 (8^85 - 1) / 7: adding it turns the digits in [-4, 4) into [0, 8)
static constexpr uint32_t SC_BIAS[8] = {0x24924924u, 0x49249249u, 0x92492492u, 0x24924924u, 0x49249249u, 0x92492492u, 0x24924924u, 0x49249249u};

BZK_HD Pt pt_identity() { return {fe_small(0), fe_small(1), fe_small(1), fe_small(0)}; }
BZK_HD Pt pt_dbl(const Pt& p) {
    const Fe xx = fe_sq(p.X), yy = fe_sq(p.Y), zz = fe_sq(p.Z), xy2 = fe_sq(fe_add(p.X, p.Y));
    const Fe ypx = fe_add(yy, xx), ymx = fe_sub(yy, xx);
    const Fe cx = fe_sub(xy2, ypx), ct = fe_sub(fe_add(zz, zz), ymx);  // completed (cx : ypx : ymx : ct)
    return {fe_mul(cx, ct), fe_mul(ypx, ymx), fe_mul(ymx, ct), fe_mul(cx, ypx)};
}
BZK_HD Cached pt_cache(const Pt& p) { return {fe_add(p.Y, p.X), fe_sub(p.Y, p.X), p.Z, fe_mul(p.T, fe_const(FE_D2))}; }
// p + q, or p - q where neg
BZK_HD Pt pt_add_cached(const Pt& p, const Cached& q, bool neg) {
    const Fe pp = fe_mul(fe_add(p.Y, p.X), fe_sel(neg, q.YmX, q.YpX)), mm = fe_mul(fe_sub(p.Y, p.X), fe_sel(neg, q.YpX, q.YmX));
    const Fe tt = fe_mul(p.T, q.T2d), zz = fe_mul(p.Z, q.Z), zz2 = fe_add(zz, zz);
    const Fe s = fe_add(zz2, tt), d = fe_sub(zz2, tt);
    const Fe cx = fe_sub(pp, mm), cy = fe_add(pp, mm), cz = fe_sel(neg, d, s), ct = fe_sel(neg, s, d);
    return {fe_mul(cx, ct), fe_mul(cy, cz), fe_mul(cz, ct), fe_mul(cx, cy)};
}
// p + an affine entry (y + x, y - x, 2 d x y)
BZK_HD Pt pt_add_niels(const Pt& p, const Fe& ypx, const Fe& ymx, const Fe& xy2d) {
    const Fe pp = fe_mul(fe_add(p.Y, p.X), ypx), mm = fe_mul(fe_sub(p.Y, p.X), ymx), tt = fe_mul(p.T, xy2d), zz2 = fe_add(p.Z, p.Z);
    const Fe cx = fe_sub(pp, mm), cy = fe_add(pp, mm), cz = fe_add(zz2, tt), ct = fe_sub(zz2, tt);
    return {fe_mul(cx, ct), fe_mul(cy, cz), fe_mul(cz, ct), fe_mul(cx, cy)};
}

// A's y (the low 255 bits of the key's words) and sign bit -> x, y; false where the radicand u / v = (y^2 - 1) / (d y^2 + 1) has no root.
// One exponentiation is inversion and root together: x = u v^3 (u v^7)^((p - 5) / 8), times sqrt(-1) where v x^2 = -u.
BZK_HD bool decode(const uint32_t (&key)[8], Fe& x, Fe& y) {
    y = fe_from_words(key);
    const Fe yy = fe_sq(y), u = fe_sub(yy, fe_small(1)), v = fe_add(fe_mul(yy, fe_const(FE_D)), fe_small(1));
    const Fe v3 = fe_mul(fe_sq(v), v), v7 = fe_mul(fe_sq(v3), v);
    x = fe_mul(fe_mul(u, v3), fe_pow22523(fe_mul(u, v7)));
    const Fe vxx = fe_mul(v, fe_sq(x));
    const bool plus = fe_is_zero(fe_sub(vxx, u)), minus = fe_is_zero(fe_add(vxx, u));
    x = fe_sel(plus, x, fe_mul(x, fe_const(FE_SQRTM1)));
    const bool flip = fe_is_negative(x) != ((key[7] >> 31) != 0);  // the non-negative root, negated where the sign bit is set
    x = fe_sel(flip, fe_neg(x), x);
    return plus || minus;
}
BZK_HD void encode(const Pt& p, uint32_t (&out)[8]) {
    const Fe zi = fe_invert(p.Z), x = fe_mul(p.X, zi), y = fe_mul(p.Y, zi);
    fe_to_words(y, out);
    out[7] |= fe_is_negative(x) ? 0x80000000u : 0;
}

BZK_HD void load_words8(const uint8_t* p, uint32_t (&w)[8]) {  // any alignment
#pragma unroll
    for (int i = 0; i < 8; ++i) __builtin_memcpy(&w[i], p + 4 * i, 4);
}
BZK_HD void fe_store(uint32_t* at, int stride, const Fe& a) {
#pragma unroll
    for (int i = 0; i < 10; ++i) at[i * stride] = a.l[i];
}
BZK_HD Fe fe_load(const uint32_t* at, int stride) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.l[i] = at[i * stride];
    return r;
}

// SHA-512(R | A | M) for the two ways a message body is given.  A sha512::Msg body (up to two ranges and a literal byte: body.p[2] / body.len[2]
// are not used) gets R and A as the ranges in front of it; a gathered body (bzk_gather.cuh) carries R | A as its first two pieces already
// (gather::signed_form with_ra), since they lie in the same record as the signed bytes.
BZK_HD sha512::Digest hash_ram(const uint8_t* pk, const uint8_t* sig, const sha512::Msg& body) {
    sha512::Msg m;
    m.p[0] = sig; m.len[0] = 32;
    m.p[1] = pk; m.len[1] = 32;
    m.p[2] = body.p[0]; m.len[2] = body.len[0];
    m.tail = body.tail;
    return sha512::sha512_one(m);
}
BZK_HD sha512::Digest hash_ram(const uint8_t*, const uint8_t*, const gather::Msg& body) { return sha512::sha512_one(body); }

// The verdict for key pk (32 bytes), signature sig (64 bytes: R | s) and the message body (see hash_ram).  base_tab: base_table_build's words.
// lane: LANE_WORDS words of the lane's own, word k at lane[k * stride] (the kernel passes its LDS column, the host a local array).
template <class Body>
BZK_HD uint8_t verify_one(const uint8_t* pk, const uint8_t* sig, const Body& body, const uint32_t* __restrict__ base_tab, uint32_t* lane,
                          int stride) {
    uint32_t key[8], r[8], s[8];
    load_words8(pk, key);
    load_words8(sig, r);
    load_words8(sig + 32, s);
    bool ok = sc_below_l(s);
    uint32_t* const kw = lane + VAR_TAB * CACHED_WORDS * stride;
    uint32_t* const sw = kw + 9 * stride;
    {
        const sha512::Digest h = hash_ram(pk, sig, body);
        uint32_t k[8];
        sc_reduce512(h.w, k);
        uint64_t carry = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // k < 2^253 and the bias < 2^255: no carry out
            const uint64_t v = (uint64_t)k[i] + SC_BIAS[i] + carry;
            kw[i * stride] = (uint32_t)v;
            carry = v >> 32;
        }
        kw[8 * stride] = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) sw[i * stride] = s[i];
    }
    {
        Fe x, y;
        ok = decode(key, x, y) && ok;
        const Fe nx = fe_neg(x);
        Pt p = {nx, y, fe_small(1), fe_mul(nx, y)};  // -A
        const Cached c1 = pt_cache(p);
#pragma unroll 1
        for (int j = 0; j < VAR_TAB; ++j) {  // j (-A) in turn
            const Cached c = pt_cache(p);
            uint32_t* at = lane + j * CACHED_WORDS * stride;
            fe_store(at, stride, c.YpX);
            fe_store(at + 10 * stride, stride, c.YmX);
            fe_store(at + 20 * stride, stride, c.Z);
            fe_store(at + 30 * stride, stride, c.T2d);
            p = pt_add_cached(p, c1, false);
        }
    }
    Pt q = pt_identity();
#pragma unroll 1
    for (int i = VAR_DIGITS - 1; i >= 0; --i) {
#pragma unroll 1
        for (int k = 0; k < 3; ++k) q = pt_dbl(q);
        const int bit = 3 * i, w = bit >> 5;
        const uint64_t two = (uint64_t)kw[w * stride] | ((uint64_t)kw[(w + 1) * stride] << 32);
        const int d = (int)((two >> (bit & 31)) & 7) - 4;
        const int mag = d < 0 ? -d : d;
        const uint32_t* at = lane + (mag ? mag - 1 : 0) * CACHED_WORDS * stride;
        const Cached c = {fe_load(at, stride), fe_load(at + 10 * stride, stride), fe_load(at + 20 * stride, stride),
                          fe_load(at + 30 * stride, stride)};
        const Pt sum = pt_add_cached(q, c, d < 0);
        q = {fe_sel(mag != 0, sum.X, q.X), fe_sel(mag != 0, sum.Y, q.Y), fe_sel(mag != 0, sum.Z, q.Z), fe_sel(mag != 0, sum.T, q.T)};
    }
#pragma unroll 1
    for (int i = 0; i < BASE_WINDOWS; ++i) {
        const uint32_t nib = (sw[(i >> 3) * stride] >> (4 * (i & 7))) & 15;
        const uint32_t* e = base_tab + ((size_t)i * BASE_ENTRIES + nib) * NIELS_WORDS;
        q = pt_add_niels(q, fe_load(e, 1), fe_load(e + 10, 1), fe_load(e + 20, 1));
    }
    uint32_t enc[8], diff = 0;
    encode(q, enc);
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= enc[i] ^ r[i];
    return (ok && diff == 0) ? 1 : 0;
}

// host only from here.  The words of j 16^i B as (y + x, y - x, 2 d x y), window-major; B = (x, 4 / 5) with x non-negative
inline void base_table_build(std::vector<uint32_t>& tab) {
    tab.assign(BASE_TAB_WORDS, 0);
    const uint32_t by[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
    Fe x, y;
    (void)decode(by, x, y);
    Pt base = {x, y, fe_small(1), fe_mul(x, y)};
    for (int i = 0; i < BASE_WINDOWS; ++i) {
        const Cached c = pt_cache(base);
        Pt e = pt_identity();
        for (int j = 0; j < BASE_ENTRIES; ++j) {
            const Fe zi = fe_invert(e.Z), ax = fe_mul(e.X, zi), ay = fe_mul(e.Y, zi);
            uint32_t* at = tab.data() + ((size_t)i * BASE_ENTRIES + j) * NIELS_WORDS;
            fe_store(at, 1, fe_add(ay, ax));
            fe_store(at + 10, 1, fe_sub(ay, ax));
            fe_store(at + 20, 1, fe_mul(fe_mul(ax, ay), fe_const(FE_D2)));
            e = pt_add_cached(e, c, false);
        }
        base = e;  // 16 times the window's base
    }
}
// the table of the host paths, built on first use
inline const uint32_t* base_table_host() {
    static const std::vector<uint32_t> tab = [] {
        std::vector<uint32_t> t;
        base_table_build(t);
        return t;
    }();
    return tab.data();
}
// verify_one with the lane's words on the stack
template <class Body>
inline uint8_t verify_host(const uint8_t* pk, const uint8_t* sig, const Body& body) {
    uint32_t lane[LANE_WORDS];
    return verify_one(pk, sig, body, base_table_host(), lane, 1);
}

}  // namespace ed25519
}  // namespace bzk
