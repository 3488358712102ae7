// n points times ONE scalar (bzk_g1_scale_batch, the re-key of a Groth16 CRS): k P for a raw G1 record, one point per lane, the scalar
// recoded once per call into a digit string that every lane reads at the same address.
//
//   k = s_0 + s_1 X^2 (mod r),  |s_m| < 2^127                         (endo::decompose2; on the subgroup X^2 (x, y) = (BETA x, -y))
//   k P = sum_i 2^i (d0_i P + d1_i X^2 P),  d0, d1 in {-1, 0, 1}      (the non-adjacent forms of |s_0| and |s_1|, signs folded in)
// so a point costs at most 128 doublings and on average 2 x 128 / 3 additions of one of  (x, +-y), (BETA x, +-y)  - no table of multiples:
// the four operands are the record, one product (BETA x, held) and a negation.  Which operand a step adds is a property of the scalar,
// never of the point: every branch below is uniform across the launch.
//
// The formulas are the complete ones of bzk_subgroup.cuh (Renes, Costello, Batina on homogeneous projective coordinates): the accumulator
// starts as the identity, P +- X^2 P may vanish (k a multiple of X^2 +- 1), and a record outside the subgroup or off the curve must not
// fault - nothing here looks at the point.  Products per point: 128 x 8 (doublings) + 85 x 11 (additions) + 1 (BETA x) + 2 (into the
// field's form) + 4 (to affine, out of the field's form): about 1 970, against about 3 000 for 255 doublings; and the inversion, on the
// device Fermat's (ScFp28::inv: about 570 more).
//
// One text, two fields: F is a base-field policy of bzk_subgroup.cuh with two more members - inv (0 -> 0) and store (canonical
// Montgomery-2^384 limbs).  ScFp28 below is the device's; the host's is bzk_subgroup_host.h's SgHFp.
#pragma once
#include "bzk_rekey.h"
#include "bzk_subgroup.cuh"

namespace bzk {
namespace sc {

// the recoded scalar as the kernel reads it: w[0] = number of steps, then one byte per step, lowest first.  Bits 0-1 of a byte: what is added
// of (x, y) - 0 nothing, 1 (x, y), 2 (x, -y); bits 2-3: the same of (BETA x, y)
static constexpr int MAX_STEPS = 128;
struct Digits {
    uint32_t w[1 + MAX_STEPS / 4];
};

// k (Montgomery, below r) -> the digit string of bzk_scale.cuh: the non-adjacent forms of the two halves of endo::decompose2, signs folded in
inline void recode(const Fr& k_mont, Digits& dg) {
    Fr kc = fe_from_mont<FrParams>(k_mont);
    uint32_t mag[2][4];
    bool neg[2];
    endo::decompose2(kc.l, mag, neg);
    memset(&dg, 0, sizeof dg);
    uint8_t* d8 = (uint8_t*)(dg.w + 1);
    uint32_t steps = 0;
    for (int m = 0; m < 2; ++m) {
        unsigned __int128 v = 0;
        for (int i = 3; i >= 0; --i) v = (v << 32) | mag[m][i];  // < 2^127: v + 1 below cannot wrap
        const bool flip = neg[m] != (m == 1);                     // the image X^2 P carries -y
        for (uint32_t i = 0; v != 0; ++i, v >>= 1) {
            if (!(v & 1)) continue;
            const bool minus_digit = (v & 3) == 3;  // digit = 2 - (v mod 4)
            if (minus_digit) v += 1;
            else v -= 1;
            d8[i] |= (uint8_t)((minus_digit != flip ? 2 : 1) << (2 * m));
            if (i + 1 > steps) steps = i + 1;
        }
    }
    dg.w[0] = steps;  // <= MAX_STEPS: the form of a value below 2^127 has at most 128 digits
    wipe_host(&kc, sizeof kc);
    wipe_host(mag, sizeof mag);
}

// p - 2 in 64-bit words, lowest first: read by a step counter that is uniform across the launch
BZK_HD constexpr uint64_t pm2_w(int i) {
    constexpr uint64_t t[6] = {0xb9feffffffffaaa9ull, 0x1eabfffeb153ffffull, 0x6730d2a0f6b0f624ull,
                               0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull, 0x1a0111ea397fe69aull};
    return t[i];
}
struct ScFp28 : sg::SgFp28 {
    // a^(p - 2) by square-and-multiply, products inlined: 380 squarings and the exponent's set bits in products, no array a lane indexes (the
    // binary GCD of fp28::inv walks its operands' limbs by a computed index, which costs a private segment).  0 -> 0.  a reduced (< 3p)
    BZK_HD static T inv(const T& a) {
        T r = a;  // bit 380 is the leading one
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int w = 5; w >= 0; w = sg::uniform(w - 1)) {
            const uint64_t e = pm2_w(w);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
            for (int b = (w == 5 ? 59 : 63); b >= 0; b = sg::uniform(b - 1)) {
                r = fp28::sqr_body(r);
                if ((e >> b) & 1) r = fp28::mul_body(r, a);
            }
        }
        return r;
    }
    BZK_HD static void store(const T& a, uint32_t* w) {
        const Fp f = fp28::from28(a);
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i] = f.l[i];
    }
};

// o = k w (24 words each; o may be w); returns 1 when the result is the identity (o is 24 zero words then).  A record of 24 zero words is
// the identity, as this function writes it
template <class F>
BZK_HD uint8_t scale_point(const uint32_t* w, const uint32_t* dig, uint32_t* o) {
    typedef sg::CurveG1<F> C;
    typedef typename F::T T;
    T x, y;
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 24; ++i) any |= w[i];
    F::load(w, x);
    F::load(w + 12, y);
    const T bx = F::mul(F::cst(endo::G1_BETA), x);
    sg::Proj<T> acc = {F::zero(), F::one(), F::zero()};
    const uint8_t* d8 = (const uint8_t*)(dig + 1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = sg::uniform((int)dig[0]) - 1; i >= 0; i = sg::uniform(i - 1)) {
        acc = sg::dbl<C>(acc);
        const int d = sg::uniform((int)d8[i]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int m = 0; m < 2; m = sg::uniform(m + 1)) {
            const int c = (d >> (2 * m)) & 3;
            if (c) acc = sg::add_affine<C>(acc, m ? bx : x, c == 2 ? F::sub(F::zero(), y) : y);
        }
    }
    if (!any) acc.Z = F::zero();
    const uint8_t inf = F::is_zero(acc.Z) ? 1 : 0;
    const T zi = F::inv(acc.Z);  // 0 for the identity: both coordinates come out as zero
    F::store(F::mul(acc.X, zi), o);
    F::store(F::mul(acc.Y, zi), o + 12);
    return inf;
}

}  // namespace sc
}  // namespace bzk
