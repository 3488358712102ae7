// Subgroup membership of BLS12-381 points (the third check of `from_uncompressed`: canonical, on the curve, of order r), one point per lane.
//
//   G1:  P is in the order-r subgroup  <=>  [X]([X] P) == (BETA x, -y)              X = |x| = 0xd201000000010000
//   G2:  P is in the order-r subgroup  <=>  [X] P      == (CX1 conj(x), CY1 conj(y))
// (Scott, eprint 2021/1130 and 2022/352, in the sign conventions of bzk_endo.cuh: the right-hand sides are endo::g1_image and
// endo::g2_image<1>, which on the subgroup ARE multiplication by X^2 and by X.)  The left-hand sides are double-and-add ladders over the
// 64 bits of X: 63 doublings and 5 additions each, two ladders on G1 and one on G2.
//
// The ladders run on points that are NOT in the subgroup - that is what the test is for - so an addition meets P = Q, P = -Q and an
// identity accumulator (an order-3 point has 2 P = -P: the first addition of its ladder gives the identity).  The formulas are therefore the
// complete ones of Renes, Costello and Batina (eprint 2015/1060, algorithms 7 and 9 for a = 0) on homogeneous projective coordinates:
// exception-free on a curve without a point of order 2, and both #E(Fp) = h1 r and #E'(Fp2) = h2 r are odd.  No case analysis, no select,
// no branch inside a ladder that depends on the point: every lane that enters one runs the same 63 + 5 steps (a record that is out of range or
// off its curve has its verdict before the ladders and leaves there - the one divergent exit).
//   Products per point: doubling 6 M + 2 S, addition 12 M (11 M
// for an affine second operand, algorithm 8);
//   G1  2 x (63 x 8 + 5 x 12) = 1128 base-field products, + 2 (into the 28-bit form) + 3 (curve equation) + 3 (image, comparison) = 1136
//   G2  63 x (6 x 3 + 2 x 2) + 5 x 11 x 3 = 1551 base-field products, + 28 (into the 28-bit form: once, per addition, once more) + 7 + 12 = 1598
//
// One text, two fields (as bzk_pairing28.cuh): F is a base-field policy - SgFp28 below (the device's 14 x 28-bit field with every product
// inlined; tests/host/subgroup_check.hip runs it on the CPU with the bound assertions of bzk_fp28.cuh on) or SgHFp (the host's 6 x 64-bit
// field: the ctx = NULL path).  Discipline of SgFp28: every value handed out is normalised and below 3p - sums and differences are
// strongly reduced, products are product outputs (< 2p) - so every operand satisfies the bounds of bzk_fp28.cuh's mul_body / sub<3>.
#pragma once
#include "bzk_endo.cuh"

namespace bzk {
namespace sg {

static constexpr uint64_t X_ABS = 0xd201000000010000ull;  // bit 63 is the leading one
static constexpr uint8_t IN_SUBGROUP = 1, OUTSIDE = 0, INVALID = 2;

// ---- the device's base field, products inlined
struct SgFp28 {
    typedef Fp28 T;
    BZK_HD static T zero() { return fp28::zero(); }
    BZK_HD static T one() { return fp28::one(); }
    BZK_HD static bool is_zero(const T& a) { return fp28::reduced_is_zero(a); }  // a normalised and < 3p: everything this policy hands out
    BZK_HD static T add(const T& a, const T& b) { return fp28::reduce(fp28::add(a, b)); }
    BZK_HD static T sub(const T& a, const T& b) { return fp28::reduce(fp28::sub<3>(a, b)); }
    BZK_HD static T mul(const T& a, const T& b) { return fp28::mul_body(a, b); }
    BZK_HD static T sqr(const T& a) { return fp28::sqr_body(a); }
    BZK_HD static T mul12(const T& a) {  // 6 a as plain limb sums (limbs < 6 x 2^28 < 2^31, value < 18p), reduced, doubled
        const T a2 = fp28::add(a, a), a3 = fp28::add(a2, a);
        const T r = fp28::reduce(fp28::add(a3, a3));
        return add(r, r);
    }
    BZK_HD static T cst(const fp28::Consts& c) { return fp28::consts_as_fp28(c); }
    // 12 x 32-bit Montgomery-2^384 limbs -> the field's form; false when the limbs are not below p
    BZK_HD static bool load(const uint32_t* w, T& out) {
        Fp a;
#pragma unroll
        for (int i = 0; i < 12; ++i) a.l[i] = w[i];
        const T r = fp28::repack_from32(a);
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i < fp28::N; ++i) borrow = (r.l[i] - fp28::P.v[i] - borrow) >> 31;  // limbs < 2^28: a negative difference sets bit 31
        out = fp28::mul_body(r, fp28::consts_as_fp28(fp28::C_IN));
        return borrow != 0;
    }
};

// ---- Fp2 = Fp[u] / (u^2 + 1) over a base-field policy
template <class F>
struct Fp2Of {
    typedef typename F::T B;
    struct T {
        B c0, c1;
    };
    BZK_HD static T zero() { return {F::zero(), F::zero()}; }
    BZK_HD static bool is_zero(const T& a) { return F::is_zero(a.c0) && F::is_zero(a.c1); }
    BZK_HD static T add(const T& a, const T& b) { return {F::add(a.c0, b.c0), F::add(a.c1, b.c1)}; }
    BZK_HD static T sub(const T& a, const T& b) { return {F::sub(a.c0, b.c0), F::sub(a.c1, b.c1)}; }
    BZK_HD static T mul(const T& a, const T& b) {  // Karatsuba: 3 base-field products
        const B aa = F::mul(a.c0, b.c0), bb = F::mul(a.c1, b.c1);
        const B s = F::mul(F::add(a.c0, a.c1), F::add(b.c0, b.c1));
        return {F::sub(aa, bb), F::sub(F::sub(s, aa), bb)};
    }
    BZK_HD static T sqr(const T& a) {  // (c0 + c1)(c0 - c1), 2 c0 c1
        const B m = F::mul(a.c0, a.c1);
        return {F::mul(F::add(a.c0, a.c1), F::sub(a.c0, a.c1)), F::add(m, m)};
    }
    BZK_HD static T conj(const T& a) { return {a.c0, F::sub(F::zero(), a.c1)}; }
};

// ---- the two curves: K = the coordinate field's operations, b3 = multiplication by 3 b, b = the curve constant
template <class F>
struct CurveG1 {  // y^2 = x^3 + 4
    typedef F K;
    typedef typename F::T E;
    BZK_HD static E b3(const E& a) { return F::mul12(a); }
    BZK_HD static E b() {
        const E two = F::add(F::one(), F::one());
        return F::add(two, two);
    }
};
template <class F>
struct CurveG2 {  // y^2 = x^3 + 4 (1 + u)
    typedef Fp2Of<F> K;
    typedef typename K::T E;
    BZK_HD static E b3(const E& a) { return {F::mul12(F::sub(a.c0, a.c1)), F::mul12(F::add(a.c0, a.c1))}; }
    BZK_HD static E b() {
        const typename F::T four = CurveG1<F>::b();
        return {four, four};
    }
};

template <class E>
struct Proj {  // (X : Y : Z), identity = (0 : 1 : 0); a point of the curve has Z = 0 only there
    E X, Y, Z;
};

// algorithm 9: 6 M + 2 S
template <class C>
BZK_HD Proj<typename C::E> dbl(const Proj<typename C::E>& p) {
    typedef typename C::K K;
    typedef typename C::E E;
    // the four products that read p first: its coordinates are dead after them
    const E xy = K::mul(p.X, p.Y);
    E t1 = K::mul(p.Y, p.Z);
    E t0 = K::sqr(p.Y);
    E t2 = C::b3(K::sqr(p.Z));
    E z3 = K::add(t0, t0);
    z3 = K::add(z3, z3);
    z3 = K::add(z3, z3);  // 8 Y^2
    E x3 = K::mul(t2, z3);
    E y3 = K::add(t0, t2);
    z3 = K::mul(t1, z3);
    t1 = K::add(t2, t2);
    t2 = K::add(t1, t2);
    t0 = K::sub(t0, t2);
    y3 = K::add(x3, K::mul(t0, y3));
    x3 = K::mul(t0, xy);
    return {K::add(x3, x3), y3, z3};
}

// algorithm 7: 12 M
template <class C>
BZK_HD Proj<typename C::E> add(const Proj<typename C::E>& p, const Proj<typename C::E>& q) {
    typedef typename C::K K;
    typedef typename C::E E;
    E t0 = K::mul(p.X, q.X), t1 = K::mul(p.Y, q.Y), t2 = K::mul(p.Z, q.Z);
    E t3 = K::mul(K::add(p.X, p.Y), K::add(q.X, q.Y));
    t3 = K::sub(t3, K::add(t0, t1));  // X1 Y2 + X2 Y1
    E t4 = K::mul(K::add(p.Y, p.Z), K::add(q.Y, q.Z));
    t4 = K::sub(t4, K::add(t1, t2));  // Y1 Z2 + Y2 Z1
    E y3 = K::mul(K::add(p.X, p.Z), K::add(q.X, q.Z));
    y3 = K::sub(y3, K::add(t0, t2));  // X1 Z2 + X2 Z1
    E x3 = K::add(t0, t0);
    t0 = K::add(x3, t0);              // 3 X1 X2
    t2 = C::b3(t2);
    E z3 = K::add(t1, t2);
    t1 = K::sub(t1, t2);
    y3 = C::b3(y3);
    x3 = K::sub(K::mul(t3, t1), K::mul(t4, y3));
    y3 = K::add(K::mul(t1, z3), K::mul(y3, t0));
    z3 = K::add(K::mul(z3, t4), K::mul(t0, t3));
    return {x3, y3, z3};
}

// algorithm 8: p + (x, y) for a finite affine (x, y), 11 M
template <class C>
BZK_HD Proj<typename C::E> add_affine(const Proj<typename C::E>& p, const typename C::E& x, const typename C::E& y) {
    typedef typename C::K K;
    typedef typename C::E E;
    E t0 = K::mul(p.X, x), t1 = K::mul(p.Y, y);
    E t3 = K::mul(K::add(x, y), K::add(p.X, p.Y));
    t3 = K::sub(t3, K::add(t0, t1));          // X1 y + x Y1
    E t4 = K::add(K::mul(y, p.Z), p.Y);       // Y1 + y Z1
    E y3 = K::add(K::mul(x, p.Z), p.X);       // X1 + x Z1
    E x3 = K::add(t0, t0);
    t0 = K::add(x3, t0);                      // 3 X1 x
    E t2 = C::b3(p.Z);
    E z3 = K::add(t1, t2);
    t1 = K::sub(t1, t2);
    y3 = C::b3(y3);
    x3 = K::sub(K::mul(t3, t1), K::mul(t4, y3));
    y3 = K::add(K::mul(t1, z3), K::mul(y3, t0));
    z3 = K::add(K::mul(z3, t4), K::mul(t0, t3));
    return {x3, y3, z3};
}

// where a ladder takes its base from: a value the lane holds (G1: 42 registers), or the record itself, read again for each of the five
// additions (G2: the 84 registers of a held base are what the kernel would otherwise spill; four more products per addition)
template <class C>
struct HeldBase {
    Proj<typename C::E> p;
    BZK_HD Proj<typename C::E> get() const { return p; }
    BZK_HD Proj<typename C::E> add_to(const Proj<typename C::E>& acc) const { return add<C>(acc, p); }
};
// this lane's index in its wavefront, computed where it is used.  A lane's record address is then a wave-uniform base plus 48 words per
// lane; held as a per-lane pointer it is two registers that nothing reads for sixty doublings (the G2 kernel: 425 registers so, 413 this way)
BZK_HD uint32_t lane_now() {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t l;
    __asm__ volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
#else
    return 0;
#endif
}
template <class F>
struct G2Record {
    typedef typename Fp2Of<F>::T E;
    // device: valid only with ONE wavefront per block (lane_now() is threadIdx.x then; subgroup.hip asserts SG_BLOCK == 64 beside the kernel)
    const uint32_t* w0;  // the record of lane 0 (on the host: the record); x.c0 | x.c1 | y.c0 | y.c1, each checked to be below p before the ladder starts
    BZK_HD const uint32_t* words() const { return w0 + (size_t)48 * lane_now(); }
    BZK_HD Proj<E> get() const {
#if defined(__HIP_DEVICE_COMPILE__)
        __asm__ volatile("" ::: "memory");  // the loads stay here: hoisted out of the ladder they would be a held base again
#endif
        const uint32_t* w = words();
        Proj<E> r;
        F::load(w, r.X.c0);
        F::load(w + 12, r.X.c1);
        F::load(w + 24, r.Y.c0);
        F::load(w + 36, r.Y.c1);
        r.Z = {F::one(), F::zero()};
        return r;
    }
    BZK_HD Proj<E> add_to(const Proj<E>& acc) const {
        const Proj<E> b = get();
        return add_affine<CurveG2<F>>(acc, b.X, b.Y);
    }
};

// a value every lane of the wavefront agrees on, said so to the compiler: the ladder's step counter then lives in a scalar register (left to
// itself the G2 kernel kept a second, per-lane copy of it for the loop's exit test - the one register it spilled)
BZK_HD int uniform(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(v);
#else
    return v;
#endif
}

// [X] base: 63 doublings, 5 additions.  The bit tested is a constant of the step, never of the point
template <class C, class Base>
BZK_HD Proj<typename C::E> mul_x(const Base& base) {
    Proj<typename C::E> acc = base.get();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 62; i >= 0; i = uniform(i - 1)) {
        acc = dbl<C>(acc);
        if ((X_ABS >> i) & 1) acc = base.add_to(acc);
    }
    return acc;
}

// r (projective) == (ix, iy) (affine, finite)
template <class C>
BZK_HD bool equals_affine(const Proj<typename C::E>& r, const typename C::E& ix, const typename C::E& iy) {
    typedef typename C::K K;
    return !K::is_zero(r.Z) && K::is_zero(K::sub(r.X, K::mul(ix, r.Z))) && K::is_zero(K::sub(r.Y, K::mul(iy, r.Z)));
}
template <class C>
BZK_HD bool on_curve(const typename C::E& x, const typename C::E& y) {
    typedef typename C::K K;
    return K::is_zero(K::sub(K::sqr(y), K::add(K::mul(K::sqr(x), x), C::b())));
}

// the verdict of one G1 record: w = x | y, 24 words
template <class F>
BZK_HD uint8_t g1_verdict(const uint32_t* w) {
    typedef CurveG1<F> C;
    typename F::T x, y;
    const bool rx = F::load(w, x), ry = F::load(w + 12, y);
    if (!(rx && ry) || !on_curve<C>(x, y)) return INVALID;
    Proj<typename F::T> acc = {x, y, F::one()};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int k = 0; k < 2; ++k) acc = mul_x<C>(HeldBase<C>{acc});
    return equals_affine<C>(acc, F::mul(F::cst(endo::G1_BETA), x), F::sub(F::zero(), y)) ? IN_SUBGROUP : OUTSIDE;
}

// the verdict of one G2 record (x.c0 | x.c1 | y.c0 | y.c1, 48 words).  w0 is the record of lane 0 of the wavefront - lane l reads the l-th record
// after it - and on the host the record itself
template <class F>
BZK_HD uint8_t g2_verdict(const uint32_t* w0) {
    typedef CurveG2<F> C;
    typedef typename C::K K;
    const G2Record<F> rec = {w0};
    {
        const uint32_t* w = rec.words();
        typename C::E x, y;
        const bool r0 = F::load(w, x.c0), r1 = F::load(w + 12, x.c1), r2 = F::load(w + 24, y.c0), r3 = F::load(w + 36, y.c1);
        if (!(r0 && r1 && r2 && r3) || !on_curve<C>(x, y)) return INVALID;
    }
    const Proj<typename C::E> acc = mul_x<C>(rec);
    const Proj<typename C::E> p = rec.get();
    const typename C::E x = p.X, y = p.Y;
    const typename C::E cx = {F::cst(endo::G2_CX1_0), F::cst(endo::G2_CX1_1)}, cy = {F::cst(endo::G2_CY1_0), F::cst(endo::G2_CY1_1)};
    return equals_affine<C>(acc, K::mul(cx, K::conj(x)), K::mul(cy, K::conj(y))) ? IN_SUBGROUP : OUTSIDE;
}

}  // namespace sg
}  // namespace bzk
