// n points times n DIFFERENT scalars (bzk_g1_mul_batch, bzk_g2_mul_batch, the powers forms and the powers-of-tau accumulator on top of them):
// k_i P_i for a raw G1 or G2 record, one point per lane, the scalar a property of the LANE.
//
//   k = s_0 + s_1 X^2 (mod r),  |s_m| < 2^127                         (endo::decompose2)
//   on the order-r subgroups  X^2 (x, y) = (BETA x, -y) on G1  and  (CX2 x, -y) on G2, CX2 in the base field (endo::g2_image<2>)
//   k P = sum_i 2^i (b0_i (x, +-y) + b1_i (c x, -+y)),  b0, b1 the plain bits of |s_0|, |s_1|, the signs folded into y
// A preparation pass writes, per row, nine words - |s_0| (4), |s_1| (4), the two signs (bit 0: s_0 negative, bit 1: s_1 negative) - and the
// multiplication runs a FIXED 128 steps whatever the scalar: the step counter is uniform across the wavefront (sg::uniform), the bit tested is the
// lane's and never goes through it.  A step is one doubling and, per half, one mixed addition taken where the lane's bit is set; lanes of a wave
// diverge inside the conditional addition and a wave pays for both additions at nearly every step:
//   G1  128 x (8 + 2 x 11) + 570 (Fermat's inversion) + a handful  =  about 4 400 base-field products per point (one-scalar kernel: about 2 540)
//   G2  three base-field products per Fp2 product (two per square), the record read again for every addition (what sg::G2Record does for the
//       subgroup check: a held base is 56 more registers), so four more products per addition and two for the image's x
// No table of multiples, no step that depends on the point's value: the formulas are the complete ones of bzk_subgroup.cuh, so the identity
// accumulator, P +- X^2 P = 0 and records outside the subgroup or off the curve run the same steps and nothing faults.
//
// One text over a group policy G (PmG1<F>, PmG2<F>) over a base-field policy F of bzk_scale.cuh: sc::ScFp28 on the device (and in
// tests/host/pmul_check.hip, bound assertions on), SgHFp for ctx = NULL.
#pragma once
#include "bzk_scale.cuh"

namespace bzk {
namespace pm {

static constexpr int ROW_WORDS = 9;  // |s_0| | |s_1| | signs
static constexpr int STEPS = 128;

// the image X^2 P on G2 is (CX2 x, CY2 y) with CX2 in the base field and CY2 = -1: what the multiplication below relies on
BZK_HD constexpr bool consts_zero(const fp28::Consts& c) {
    for (int i = 0; i < fp28::N; ++i)
        if (c.v[i] != 0) return false;
    return true;
}
BZK_HD constexpr bool consts_equal(const fp28::Consts& a, const fp28::Consts& b) {
    for (int i = 0; i < fp28::N; ++i)
        if (a.v[i] != b.v[i]) return false;
    return true;
}
static_assert(consts_zero(endo::G2_CX2_1) && consts_zero(endo::G2_CY2_1) && consts_equal(endo::G2_CY2_0, endo::FP_MINUS1),
              "X^2 on G2 must be a base-field factor on x and a negation of y");

// canonical k < r -> the nine words of a row
BZK_HD void row_of(const uint32_t k[8], uint32_t row[ROW_WORDS]) {
    uint32_t mag[2][4];
    bool neg[2];
    endo::decompose2(k, mag, neg);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        row[i] = mag[0][i];
        row[4 + i] = mag[1][i];
    }
    row[8] = (neg[0] ? 1u : 0u) | (neg[1] ? 2u : 0u);
}
BZK_HD bool below_r(const Fr& a) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)a.l[i] - FrParams::MOD[i] - borrow;
        borrow = (uint32_t)(d >> 63);
    }
    return borrow != 0;
}
// c s^e from tab[j] = s^(2^j), j < 64 (all Montgomery): the product of the entries at the set bits of e
BZK_HD Fr power_of(const Fr& c, const Fr* tab, uint64_t e) {
    Fr acc = c;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int j = 0; j < 64; ++j)
        if ((e >> j) & 1) acc = fe_mul<FrParams>(acc, tab[j]);
    return acc;
}

// ---- the two groups.  words(): this lane's record from the pointer the kernel hands in (G1: the lane's own; G2 on the device: the record of
// lane 0 of the wavefront, the lane index taken where it is used - sg::lane_now, one wavefront per block)
template <class F>
struct PmG1 {
    typedef sg::CurveG1<F> C;
    typedef typename F::T E;
    static constexpr int WORDS = 24;
    static constexpr bool ROLLED_HALVES = false;  // the two additions of a step written out: 276 registers against 311 as a loop of two
    BZK_HD static const uint32_t* words(const uint32_t* w) { return w; }
    BZK_HD static uint32_t* words(uint32_t* w) { return w; }
    struct Base {  // held: 28 registers
        E x, y;
        BZK_HD explicit Base(const uint32_t* w) {
            F::load(w, x);
            F::load(w + 12, y);
        }
        BZK_HD void get(E& ox, E& oy) const {
            ox = x;
            oy = y;
        }
    };
    BZK_HD static E one() { return F::one(); }
    BZK_HD static E image_x(const E& x) { return F::mul(F::cst(endo::G1_BETA), x); }
    BZK_HD static E neg(const E& a) { return F::sub(F::zero(), a); }
    BZK_HD static E inv(const E& a) { return F::inv(a); }
    BZK_HD static void store(const E& a, uint32_t* o) { F::store(a, o); }
};
template <class F>
struct PmG2 {
    typedef sg::CurveG2<F> C;
    typedef typename C::E E;
    static constexpr int WORDS = 48;
    static constexpr bool ROLLED_HALVES = true;  // one addition's code for both halves: 499 registers and 9 spills against 511 and 26 written out
    BZK_HD static const uint32_t* words(const uint32_t* w) { return w + (size_t)48 * sg::lane_now(); }
    BZK_HD static uint32_t* words(uint32_t* w) { return w + (size_t)48 * sg::lane_now(); }
    struct Base {  // read again for every addition
        sg::G2Record<F> rec;
        BZK_HD explicit Base(const uint32_t* w0) : rec{w0} {}
        BZK_HD void get(E& ox, E& oy) const {
            const sg::Proj<E> p = rec.get();
            ox = p.X;
            oy = p.Y;
        }
    };
    BZK_HD static E one() { return {F::one(), F::zero()}; }
    BZK_HD static E image_x(const E& x) {
        const typename F::T c = F::cst(endo::G2_CX2_0);
        return {F::mul(c, x.c0), F::mul(c, x.c1)};
    }
    BZK_HD static E neg(const E& a) { return {F::sub(F::zero(), a.c0), F::sub(F::zero(), a.c1)}; }
    BZK_HD static E inv(const E& a) {  // conj(a) / (c0^2 + c1^2); 0 -> 0
        const typename F::T n = F::inv(F::add(F::sqr(a.c0), F::sqr(a.c1)));
        return {F::mul(a.c0, n), F::sub(F::zero(), F::mul(a.c1, n))};
    }
    BZK_HD static void store(const E& a, uint32_t* o) {
        F::store(a.c0, o);
        F::store(a.c1, o + 12);
    }
};

// one half of a step: acc += (x, +-y) for h = 0, (c x, -+y) for h = 1, where this lane's bit is set.  h is uniform, bit is the lane's
template <class G>
BZK_HD void add_half(sg::Proj<typename G::C::E>& acc, const typename G::Base& base, uint32_t bit, int h, uint32_t sgn) {
    typedef typename G::C::E E;
    if (!bit) return;
    E x, y;
    base.get(x, y);
    if (h) x = G::image_x(x);
    if ((((sgn >> h) ^ (uint32_t)h) & 1) != 0) y = G::neg(y);  // the image carries -y
    acc = sg::add_affine<typename G::C>(acc, x, y);
}

// o = k w for the row of k (o may be w: the record's last read is before the first store); returns 1 when the result is the identity (o is
// zero words then).  A record of zero words is the identity
template <class G>
BZK_HD uint8_t mul_point(const uint32_t* w0, const uint32_t* row, uint32_t* o0) {
    typedef typename G::C C;
    typedef typename C::K K;
    typedef typename C::E E;
    uint32_t any = 0;
    {
        const uint32_t* w = G::words(w0);
#pragma unroll
        for (int i = 0; i < G::WORDS; ++i) any |= w[i];
    }
    const typename G::Base base(w0);
    const uint32_t sgn = row[8];
    sg::Proj<E> acc = {K::zero(), G::one(), K::zero()};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int wd = 3; wd >= 0; wd = sg::uniform(wd - 1)) {
        const uint32_t m0 = row[wd], m1 = row[4 + wd];  // this lane's: never through sg::uniform
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
        for (int b = 31; b >= 0; b = sg::uniform(b - 1)) {
            acc = sg::dbl<C>(acc);
            if (G::ROLLED_HALVES) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
                for (int h = 0; h < 2; h = sg::uniform(h + 1)) add_half<G>(acc, base, ((h ? m1 : m0) >> b) & 1, h, sgn);
            } else {
                add_half<G>(acc, base, (m0 >> b) & 1, 0, sgn);
                add_half<G>(acc, base, (m1 >> b) & 1, 1, sgn);
            }
        }
    }
    if (!any) acc.Z = K::zero();
    const uint8_t inf = K::is_zero(acc.Z) ? 1 : 0;
    const E zi = G::inv(acc.Z);  // 0 for the identity: both coordinates come out as zero
    uint32_t* o = G::words(o0);
    G::store(K::mul(acc.X, zi), o);
    G::store(K::mul(acc.Y, zi), o + G::WORDS / 2);
    return inf;
}

}  // namespace pm
}  // namespace bzk
