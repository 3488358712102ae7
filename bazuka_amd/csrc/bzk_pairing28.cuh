// The BLS12-381 pairing tower and the three per-proof steps of a Groth16 verification, generic over the field operations: instantiated over the
// host's 64-bit-limb field (HFpOps / HFp2Ops: host_pairing.h, `bzk_groth16_verify` and the ctx = NULL path of `bzk_groth16_verify_batch`) and over
// the device's 14 x 28-bit field (Fp28Ops below / Fp2x28Ops: verify.hip's kernels, and tests/host/pairing28_check.hip on the CPU with bound
// assertions).  One text, two fields.
//
//   values   Fp2 / Fp6 arithmetic works on values (Tower<F1, F2>): an Fp6 element is 84 dwords on the device and the formulas run in registers.
//   slots    An Fp12 value (168 dwords) does not: Fp12-level functions work on SLOTS of a per-proof slab, addressed through a lane policy L
//            (l.ld1(i) / l.st1(i, v): the i-th base-field element of this proof's slab).  On the device the slab is a limb-major region of the
//            call's workspace (word w of slot i of lane t at slab[(14 i + w) stride + t]: a wavefront's access is one coalesced row); on the
//            host it is a local array.  Slot functions are real calls on the device (BZK_PFN: each Fp6 product is ~6 k instructions - inlined
//            at every use the Miller loop alone would be several instruction caches long) and take the lane by value: a pointer into the
//            workspace and slot numbers, never an address of the caller's private data.
//   bounds   every value handed out is normalised and below 3p (sums, differences: `reduce`) or an Fp2 product (components below 8p) - the
//            discipline Fp2x28Ops documents, under which every F1::mul / F2::mul operand here satisfies the bounds of bzk_fp28.cuh.
#pragma once
#include "bzk_fp28.cuh"

#if defined(__HIP_DEVICE_COMPILE__)
#define BZK_PFN __host__ __device__ __noinline__
#else
#define BZK_PFN __host__ __device__ inline
#endif

namespace bzk {

// the HFpOps interface on Fp28, same discipline as Fp2x28Ops: sums and differences strongly reduced (< 3p), products product outputs (< 2p)
struct Fp28Ops {
    typedef Fp28 T;
    static constexpr int LIMBS = 14;
    BZK_HD static T zero() { return fp28::zero(); }
    BZK_HD static T one() { return fp28::one(); }
    BZK_HD static bool is_zero(const T& a) { return fp28::reduced_is_zero(fp28::reduce(a)); }
    BZK_HD static T add(const T& a, const T& b) { return fp28::reduce(fp28::add(a, b)); }
    BZK_HD static T sub(const T& a, const T& b) { return fp28::reduce(fp28::sub<12>(a, b)); }   // b normalised, < 12p
    BZK_HD static T neg(const T& a) { return sub(zero(), a); }
    BZK_HD static T dbl(const T& a) { return add(a, a); }
    BZK_HD static T mul(const T& a, const T& b) { return fp28::mul(a, b); }
    BZK_HD static T sqr(const T& a) { return fp28::sqr(a); }
    BZK_HD static T inv(const T& a) { return fp28::inv(a); }
    BZK_HD static bool eq(const T& a, const T& b) { return is_zero(sub(a, b)); }
};

namespace pairing {

static constexpr uint64_t X_ABS = 0xd201000000010000ull;   // |x| of the curve; bit 63 is the leading one
static constexpr int MILLER_STEPS = 63 + 5;                // doublings + additions: lines per pair

// ---- Fp2 / Fp6 on values
template <class F1_, class F2_>
struct Tower {
    typedef F1_ F1;
    typedef F2_ F2;
    typedef typename F1::T E1;
    typedef typename F2::T E2;
    struct E6 { E2 c0, c1, c2; };
    struct E12 { E6 a0, a1; };
    struct G2J { E2 X, Y, Z; };

    BZK_HD static E2 e2_mul_xi(const E2& a) { return {F1::sub(a.c0, a.c1), F1::add(a.c0, a.c1)}; }  // * (1 + u)
    BZK_HD static E2 e2_scale(const E2& a, const E1& k) { return {F1::mul(a.c0, k), F1::mul(a.c1, k)}; }
    BZK_HD static E2 e2_conj(const E2& a) { return {a.c0, F1::neg(a.c1)}; }
    BZK_HD static E6 e6_zero() { return {F2::zero(), F2::zero(), F2::zero()}; }
    BZK_HD static E6 e6_one() { return {F2::one(), F2::zero(), F2::zero()}; }
    BZK_HD static E6 e6_add(const E6& a, const E6& b) { return {F2::add(a.c0, b.c0), F2::add(a.c1, b.c1), F2::add(a.c2, b.c2)}; }
    BZK_HD static E6 e6_sub(const E6& a, const E6& b) { return {F2::sub(a.c0, b.c0), F2::sub(a.c1, b.c1), F2::sub(a.c2, b.c2)}; }
    BZK_HD static E6 e6_neg(const E6& a) { return {F2::neg(a.c0), F2::neg(a.c1), F2::neg(a.c2)}; }
    BZK_HD static E6 e6_mul(const E6& a, const E6& b) {  // Karatsuba: 6 Fp2 products
        const E2 t0 = F2::mul(a.c0, b.c0), t1 = F2::mul(a.c1, b.c1), t2 = F2::mul(a.c2, b.c2);
        E6 r;
        r.c0 = F2::add(t0, e2_mul_xi(F2::sub(F2::sub(F2::mul(F2::add(a.c1, a.c2), F2::add(b.c1, b.c2)), t1), t2)));
        r.c1 = F2::add(F2::sub(F2::sub(F2::mul(F2::add(a.c0, a.c1), F2::add(b.c0, b.c1)), t0), t1), e2_mul_xi(t2));
        r.c2 = F2::add(F2::sub(F2::sub(F2::mul(F2::add(a.c0, a.c2), F2::add(b.c0, b.c2)), t0), t2), t1);
        return r;
    }
    BZK_HD static E6 e6_mul_v(const E6& a) { return {e2_mul_xi(a.c2), a.c0, a.c1}; }
    // a * (b0 + b1 v)
    BZK_HD static E6 e6_mul_by_01(const E6& a, const E2& b0, const E2& b1) {
        return {F2::add(F2::mul(a.c0, b0), e2_mul_xi(F2::mul(a.c2, b1))), F2::add(F2::mul(a.c0, b1), F2::mul(a.c1, b0)),
                F2::add(F2::mul(a.c1, b1), F2::mul(a.c2, b0))};
    }
    // a * (k v) with k in Fp
    BZK_HD static E6 e6_mul_by_1_fp(const E6& a, const E1& k) { return {e2_mul_xi(e2_scale(a.c2, k)), e2_scale(a.c0, k), e2_scale(a.c1, k)}; }
    // a * (b1 v)
    BZK_HD static E6 e6_mul_by_1(const E6& a, const E2& b1) { return {e2_mul_xi(F2::mul(a.c2, b1)), F2::mul(a.c0, b1), F2::mul(a.c1, b1)}; }
    BZK_HD static E6 e6_inv(const E6& a) {
        const E2 c0 = F2::sub(F2::sqr(a.c0), e2_mul_xi(F2::mul(a.c1, a.c2)));
        const E2 c1 = F2::sub(e2_mul_xi(F2::sqr(a.c2)), F2::mul(a.c0, a.c1));
        const E2 c2 = F2::sub(F2::sqr(a.c1), F2::mul(a.c0, a.c2));
        const E2 t = F2::add(F2::mul(a.c0, c0), e2_mul_xi(F2::add(F2::mul(a.c2, c1), F2::mul(a.c1, c2))));
        const E2 ti = F2::inv(t);
        return {F2::mul(c0, ti), F2::mul(c1, ti), F2::mul(c2, ti)};
    }
    BZK_HD static bool e6_eq(const E6& a, const E6& b) { return F2::eq(a.c0, b.c0) && F2::eq(a.c1, b.c1) && F2::eq(a.c2, b.c2); }
    // (a + b t)^2 = a^2 + xi b^2 + ((a + b)^2 - a^2 - b^2) t  in Fp4 = Fp2[t] / (t^2 - xi)
    BZK_HD static void fp4_sqr(const E2& a, const E2& b, E2& o0, E2& o1) {
        const E2 t0 = F2::sqr(a), t1 = F2::sqr(b);
        o0 = F2::add(e2_mul_xi(t1), t0);
        o1 = F2::sub(F2::sub(F2::sqr(F2::add(a, b)), t0), t1);
    }
    BZK_HD static E2 three_minus_two(const E2& sq, const E2& v) { const E2 d = F2::sub(sq, v); return F2::add(F2::add(d, d), sq); }   // 3 sq - 2 v
    BZK_HD static E2 three_plus_two(const E2& sq, const E2& v) { const E2 d = F2::add(sq, v); return F2::add(F2::add(d, d), sq); }     // 3 sq + 2 v

    // ---- one step of a Miller loop's running point T (Jacobian, twist coordinates) with the line through it, as the three coefficients
    //     l00 + (cx xP) w^2 + (cy yP) w^3
    // of the affine line scaled by its slope's denominator (an Fp2 factor the final exponentiation removes).  They depend on Q only, never on
    // P: for a fixed Q they are a table.  false = the slope's denominator is zero (T of order 2, or T = +-Q): T and the outputs are untouched.
    //   doubling  lam = 3 X^2 / (2 Y Z),          x 2 Y Z^3:   (3 X^3 - 2 Y^2)  -  3 X^2 Z^2 xP w^2  +  2 Y Z^3 yP w^3
    //   addition  lam = (yQ Z^3 - Y) / (Z H),     x Z H:       (R xQ - yQ Z H)  -  R xP w^2          +  Z H yP w^3       H = xQ Z^2 - X, R = yQ Z^3 - Y
    BZK_HD static bool dbl_coeffs(G2J& T, E2& l00, E2& cx, E2& cy) {
        if (F2::is_zero(T.Y)) return false;   // vertical tangent (Z is never zero before this happens)
        const E2 A = F2::sqr(T.X), B = F2::sqr(T.Y), C = F2::sqr(B), ZZ = F2::sqr(T.Z);
        const E2 E = F2::add(F2::add(A, A), A);                                          // 3 X^2
        E2 D = F2::sub(F2::sub(F2::sqr(F2::add(T.X, B)), A), C);
        D = F2::add(D, D);                                                               // 4 X Y^2
        const E2 Z3 = F2::sub(F2::sub(F2::sqr(F2::add(T.Y, T.Z)), B), ZZ);               // 2 Y Z
        l00 = F2::sub(F2::mul(E, T.X), F2::add(B, B));                                   // 3 X^3 - 2 Y^2
        cx = F2::neg(F2::mul(E, ZZ));                                                    // - 3 X^2 Z^2
        cy = F2::mul(Z3, ZZ);                                                            // 2 Y Z^3
        const E2 X3 = F2::sub(F2::sqr(E), F2::add(D, D));
        E2 C8 = F2::add(C, C);
        C8 = F2::add(C8, C8);
        C8 = F2::add(C8, C8);
        T = {X3, F2::sub(F2::mul(E, F2::sub(D, X3)), C8), Z3};
        return true;
    }
    BZK_HD static bool add_coeffs(G2J& T, const E2& Qx, const E2& Qy, E2& l00, E2& cx, E2& cy) {
        const E2 ZZ = F2::sqr(T.Z);
        const E2 H = F2::sub(F2::mul(Qx, ZZ), T.X);
        const E2 Rr = F2::sub(F2::mul(Qy, F2::mul(ZZ, T.Z)), T.Y);
        if (F2::is_zero(H)) return false;                                                // T = +-Q
        const E2 Z3 = F2::mul(T.Z, H);
        l00 = F2::sub(F2::mul(Rr, Qx), F2::mul(Qy, Z3));
        cx = F2::neg(Rr);
        cy = Z3;
        const E2 HH = F2::sqr(H), HHH = F2::mul(HH, H), V = F2::mul(T.X, HH);
        const E2 X3 = F2::sub(F2::sub(F2::sqr(Rr), HHH), F2::add(V, V));
        T = {X3, F2::sub(F2::mul(Rr, F2::sub(V, X3)), F2::mul(T.Y, HHH)), Z3};
        return true;
    }
};

// ---- lanes.  The device lane (also run on the CPU by the harness, where stride is whatever the test picks)
struct Lane28 {
    typedef Fp28Ops F1;
    typedef Fp2x28Ops F2;
    uint32_t* p;       // word 0 of slot 0 of this proof
    uint32_t stride;   // words between consecutive words of a slot
    BZK_HD Fp28 ld1(int i) const {
        Fp28 r;
        const uint32_t* q = p + (size_t)(14 * i) * stride;
#pragma unroll
        for (int w = 0; w < 14; ++w) r.l[w] = q[(size_t)w * stride];
        return r;
    }
    BZK_HD void st1(int i, const Fp28& v) const {
        uint32_t* q = p + (size_t)(14 * i) * stride;
#pragma unroll
        for (int w = 0; w < 14; ++w) q[(size_t)w * stride] = v.l[w];
    }
};

// slot numbers of a proof's slab, in base-field elements.  F and R1..R5 hold Fp12 values, TMP three Fp6 temporaries; the Miller loop keeps its
// points where the final exponentiation later keeps R1..R2
namespace slot {
static constexpr int F = 0, R1 = 12, R2 = 24, R3 = 36, R4 = 48, R5 = 60, TMP = 72, COUNT = 90;
static constexpr int PA = 12, PX = 14, PC = 16, QB = 18, TT = 22, LINE = 28;   // A, X, C (x, y); B (x, y in Fp2); running point (X, Y, Z); a line
}  // namespace slot

// what prepare_one leaves for the other two steps
static constexpr uint32_t FLAG_REFUSED = 1, FLAG_AB = 2, FLAG_X = 4, FLAG_C = 8, FLAG_DEGENERATE = 16;

template <class L> BZK_HD typename L::F2::T ld2(const L& l, int s) { return {l.ld1(s), l.ld1(s + 1)}; }
template <class L> BZK_HD void st2(const L& l, int s, const typename L::F2::T& v) { l.st1(s, v.c0); l.st1(s + 1, v.c1); }
template <class L> BZK_HD typename Tower<typename L::F1, typename L::F2>::E6 ld6(const L& l, int s) { return {ld2(l, s), ld2(l, s + 2), ld2(l, s + 4)}; }
template <class L> BZK_HD void st6(const L& l, int s, const typename Tower<typename L::F1, typename L::F2>::E6& v) {
    st2(l, s, v.c0); st2(l, s + 2, v.c1); st2(l, s + 4, v.c2);
}
#define BZK_TW typedef Tower<typename L::F1, typename L::F2> T; typedef typename T::E2 E2; typedef typename T::E6 E6; typedef typename L::F2 F2; typedef typename L::F1 F1

// ---- Fp6 on slots (every function reads all it needs before it writes: a destination may be an operand)
template <class L> BZK_PFN void s6_mul(L l, int d, int a, int b) { BZK_TW; st6(l, d, T::e6_mul(ld6(l, a), ld6(l, b))); }
// d = (a0 + a1)(b0 + b1) - t0 - t1
template <class L> BZK_PFN void s6_mul_sum(L l, int d, int a0, int a1, int b0, int b1, int t0, int t1) {
    BZK_TW;
    const E6 m = T::e6_mul(T::e6_add(ld6(l, a0), ld6(l, a1)), T::e6_add(ld6(l, b0), ld6(l, b1)));
    st6(l, d, T::e6_sub(T::e6_sub(m, ld6(l, t0)), ld6(l, t1)));
}
template <class L> BZK_PFN void s6_add_mulv(L l, int d, int a, int b) { BZK_TW; st6(l, d, T::e6_add(ld6(l, a), T::e6_mul_v(ld6(l, b)))); }   // a + v b
template <class L> BZK_PFN void s6_sub_mulv(L l, int d, int a, int b) { BZK_TW; st6(l, d, T::e6_sub(ld6(l, a), T::e6_mul_v(ld6(l, b)))); }   // a - v b
template <class L> BZK_PFN void s6_inv(L l, int d, int a) { BZK_TW; st6(l, d, T::e6_inv(ld6(l, a))); }
template <class L> BZK_PFN void s6_neg(L l, int d, int a) { BZK_TW; st6(l, d, T::e6_neg(ld6(l, a))); }
template <class L> BZK_HD void s6_copy(const L& l, int d, int a) {
    if (d == a) return;
#pragma unroll 1
    for (int i = 0; i < 6; ++i) l.st1(d + i, l.ld1(a + i));
}
template <class L> BZK_HD void s12_copy(const L& l, int d, int a) { s6_copy(l, d, a); s6_copy(l, d + 6, a + 6); }

// ---- Fp12 on slots; t: 12 (e12_mul, e12_sqr, e12_inv, e12_mul_by_014) free slots for temporaries
template <class L> BZK_HD void e12_set_one(const L& l, int d) {
    l.st1(d, L::F1::one());
#pragma unroll 1
    for (int i = 1; i < 12; ++i) l.st1(d + i, L::F1::zero());
}
template <class L> BZK_HD void e12_mul(const L& l, int d, int a, int b, int t) {
    s6_mul(l, t, a, b);
    s6_mul(l, t + 6, a + 6, b + 6);
    s6_mul_sum(l, d + 6, a, a + 6, b, b + 6, t, t + 6);
    s6_add_mulv(l, d, t, t + 6);
}
// (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - ab - v ab + 2 ab w,  ab = a0 a1 (in slot t)
template <class L> BZK_PFN void s12_sqr_tail(L l, int d, int a, int t) {
    BZK_TW;
    const E6 a0 = ld6(l, a), a1 = ld6(l, a + 6);
    const E6 m = T::e6_mul(T::e6_add(a0, a1), T::e6_add(a0, T::e6_mul_v(a1)));
    const E6 ab = ld6(l, t);
    st6(l, d, T::e6_sub(T::e6_sub(m, ab), T::e6_mul_v(ab)));
    st6(l, d + 6, T::e6_add(ab, ab));
}
template <class L> BZK_HD void e12_sqr(const L& l, int d, int a, int t) {
    s6_mul(l, t, a, a + 6);
    s12_sqr_tail(l, d, a, t);
}
template <class L> BZK_HD void e12_conj(const L& l, int d, int a) {
    s6_copy(l, d, a);
    s6_neg(l, d + 6, a + 6);
}
template <class L> BZK_HD void e12_inv(const L& l, int d, int a, int t) {   // d is not a
    s6_mul(l, t, a, a);
    s6_mul(l, t + 6, a + 6, a + 6);
    s6_sub_mulv(l, t, t, t + 6);
    s6_inv(l, t, t);
    s6_mul(l, d, a, t);
    s6_mul(l, d + 6, a + 6, t);
    s6_neg(l, d + 6, d + 6);
}
template <class L> BZK_PFN bool e12_is_one(L l, int a) {
    BZK_TW;
    bool ok = F2::eq(ld2(l, a), F2::one());
#pragma unroll 1
    for (int i = 2; i < 12; i += 2) ok = F2::is_zero(ld2(l, a + i)) && ok;
    return ok;
}
// f *= c0 + c1 v + (c4 v) w, the three coefficients in slots line, line + 2, line + 4: positions 0, 1 and 4 of the tower, 6 + 3 + 6 Fp2 products
template <class L> BZK_PFN void s014_a(L l, int d, int f, int line) { BZK_TW; st6(l, d, T::e6_mul_by_01(ld6(l, f), ld2(l, line), ld2(l, line + 2))); }
template <class L> BZK_PFN void s014_b(L l, int d, int f1, int line) { BZK_TW; st6(l, d, T::e6_mul_by_1(ld6(l, f1), ld2(l, line + 4))); }
template <class L> BZK_PFN void s014_c(L l, int f, int line, int t) {
    BZK_TW;
    const E6 m = T::e6_mul_by_01(T::e6_add(ld6(l, f), ld6(l, f + 6)), ld2(l, line), F2::add(ld2(l, line + 2), ld2(l, line + 4)));
    st6(l, f + 6, T::e6_sub(T::e6_sub(m, ld6(l, t)), ld6(l, t + 6)));
}
template <class L> BZK_HD void e12_mul_by_014(const L& l, int f, int line, int t) {
    s014_a(l, t, f, line);
    s014_b(l, t + 6, f + 6, line);
    s014_c(l, f, line, t);
    s6_add_mulv(l, f, t, t + 6);
}
// Frobenius: (sum_i c_i w^i)^p = sum_i conj(c_i) gamma_i w^i,  gamma_i = xi^(i (p - 1) / 6) at g[i] (g[0] = 1 is not read)
template <class L> BZK_PFN void e12_frob(L l, int d, int a, const typename L::F2::T* g) {
    BZK_TW;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
        const int s = (k & 1) * 6 + (k >> 1) * 2;   // w^k: a0.c0, a1.c0, a0.c1, a1.c1, a0.c2, a1.c2
        E2 c = T::e2_conj(ld2(l, a + s));
        if (k) c = F2::mul(c, g[k]);
        st2(l, d + s, c);
    }
}
// squaring in the cyclotomic subgroup (Granger - Scott): three squarings in Fp4 over the pairs (c0, c3), (c1, c4), (c2, c5) of f = sum c_i w^i
// regrouped as g = x + y s + z s^2 over Fp4 (s = w, s^3 = t), unitary:  g^2 = (3 x^2 - 2 conj x) + (3 t z^2 + 2 conj y) s + (3 y^2 - 2 conj z) s^2
template <class L> BZK_PFN void s_cyc_sqr_x(L l, int d, int a) {   // w^0 and w^3
    BZK_TW;
    const E2 c0 = ld2(l, a), c3 = ld2(l, a + 8);
    E2 A0, A1;
    T::fp4_sqr(c0, c3, A0, A1);
    st2(l, d, T::three_minus_two(A0, c0));
    st2(l, d + 8, T::three_plus_two(A1, c3));
}
template <class L> BZK_PFN void s_cyc_sqr_yz(L l, int d, int a) {   // w^1, w^2, w^4, w^5
    BZK_TW;
    const E2 c1 = ld2(l, a + 6), c2 = ld2(l, a + 2), c4 = ld2(l, a + 4), c5 = ld2(l, a + 10);
    E2 B0, B1, C0, C1;
    T::fp4_sqr(c1, c4, B0, B1);
    T::fp4_sqr(c2, c5, C0, C1);
    st2(l, d + 6, T::three_plus_two(T::e2_mul_xi(C1), c1));   // w^1: 3 xi C1 + 2 c1
    st2(l, d + 4, T::three_minus_two(C0, c4));                // w^4: 3 C0 - 2 c4
    st2(l, d + 2, T::three_minus_two(B0, c2));                // w^2: 3 B0 - 2 c2
    st2(l, d + 10, T::three_plus_two(B1, c5));                // w^5: 3 B1 + 2 c5
}
template <class L> BZK_HD void e12_cyc_sqr(const L& l, int d, int a) {
    s_cyc_sqr_x(l, d, a);
    s_cyc_sqr_yz(l, d, a);
}
// g^x for g in the cyclotomic subgroup (x = -|x|: the inverse there is the conjugate); d is not g
template <class L> BZK_HD void e12_cyc_exp_x(const L& l, int d, int g, int t) {
    s12_copy(l, d, g);
#pragma unroll 1
    for (int i = 62; i >= 0; --i) {
        e12_cyc_sqr(l, d, d);
        if ((X_ABS >> i) & 1) e12_mul(l, d, d, g, t);
    }
    e12_conj(l, d, d);
}
// f^(p^6 - 1)(p^2 + 1) of the value in slot F, left in R1; uses R2, R3, TMP
template <class L> BZK_HD void final_exp_easy(const L& l, const typename L::F2::T* frob) {
    using namespace slot;
    e12_inv(l, R1, F, TMP);
    e12_conj(l, R2, F);
    e12_mul(l, R3, R2, R1, TMP);     // g = f^(p^6 - 1)
    e12_frob(l, R1, R3, frob);
    e12_frob(l, R2, R1, frob);
    e12_mul(l, R1, R2, R3, TMP);     // ^(p^2 + 1)
}
// (easy part)^( (x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3 ) = f^(3 (p^12 - 1) / r) of the value in slot F, left in R4
template <class L> BZK_HD void final_exp(const L& l, const typename L::F2::T* frob) {
    using namespace slot;
    final_exp_easy(l, frob);                                         // m in R1
    e12_cyc_exp_x(l, R2, R1, TMP); e12_conj(l, R3, R1); e12_mul(l, R2, R2, R3, TMP);   // t = m^(x - 1) in R2
    e12_cyc_exp_x(l, R3, R2, TMP); e12_conj(l, R4, R2); e12_mul(l, R3, R3, R4, TMP);   // a = m^((x - 1)^2) in R3
    e12_cyc_exp_x(l, R2, R3, TMP); e12_frob(l, R4, R3, frob); e12_mul(l, R2, R2, R4, TMP);   // b = a^(x + p) in R2
    e12_cyc_exp_x(l, R3, R2, TMP); e12_cyc_exp_x(l, R4, R3, TMP);                      // b^(x^2) in R4
    e12_frob(l, R3, R2, frob); e12_frob(l, R5, R3, frob); e12_mul(l, R4, R4, R5, TMP); // * b^(p^2)
    e12_conj(l, R3, R2); e12_mul(l, R4, R4, R3, TMP);                                  // c = b^(x^2 + p^2 - 1) in R4
    e12_cyc_sqr(l, R2, R1); e12_mul(l, R2, R2, R1, TMP); e12_mul(l, R4, R4, R2, TMP);  // * m^3
}

// ---- Miller steps on slots: the running point in tt (X, Y, Z), P = (x, y) in sp, the line left in `line`; false = degenerate
template <class L> BZK_PFN bool s_dbl_step(L l, int tt, int sp, int line) {
    BZK_TW;
    typename T::G2J P = {ld2(l, tt), ld2(l, tt + 2), ld2(l, tt + 4)};
    E2 l00, cx, cy;
    if (!T::dbl_coeffs(P, l00, cx, cy)) return false;
    st2(l, line, l00);
    st2(l, line + 2, T::e2_scale(cx, l.ld1(sp)));
    st2(l, line + 4, T::e2_scale(cy, l.ld1(sp + 1)));
    st2(l, tt, P.X); st2(l, tt + 2, P.Y); st2(l, tt + 4, P.Z);
    return true;
}
template <class L> BZK_PFN bool s_add_step(L l, int tt, int sq, int sp, int line) {
    BZK_TW;
    typename T::G2J P = {ld2(l, tt), ld2(l, tt + 2), ld2(l, tt + 4)};
    E2 l00, cx, cy;
    if (!T::add_coeffs(P, ld2(l, sq), ld2(l, sq + 2), l00, cx, cy)) return false;
    st2(l, line, l00);
    st2(l, line + 2, T::e2_scale(cx, l.ld1(sp)));
    st2(l, line + 4, T::e2_scale(cy, l.ld1(sp + 1)));
    st2(l, tt, P.X); st2(l, tt + 2, P.Y); st2(l, tt + 4, P.Z);
    return true;
}
// the line of a FIXED second argument from its table entry (l00, cx, cy): two scalings
template <class L> BZK_PFN void s_fixed_line(L l, int line, const typename L::F2::T* c, int sp) {
    BZK_TW;
    st2(l, line, c[0]);
    st2(l, line + 2, T::e2_scale(c[1], l.ld1(sp)));
    st2(l, line + 4, T::e2_scale(c[2], l.ld1(sp + 1)));
}

// ---- a verifying key as the per-proof steps read it (pointers into host memory, or into the call's workspace on the device)
template <class F1, class F2>
struct KeyView {
    uint32_t n_inputs;
    const typename F1::T* tab_xy;    // (15 n_inputs + 1) x (x, y): entry 15 i + j - 1 = j IC_(i + 1) affine, the last one IC_0
    const uint8_t* tab_inf;          // 15 n_inputs + 1: 1 = that entry is the identity
    const typename F2::T* gamma;     // MILLER_STEPS x (l00, cx, cy) of -gamma
    const typename F2::T* delta;     // the same of -delta
    const typename F1::T* m;         // 12: multi_miller({-alpha}, {beta})
    const typename F2::T* frob;      // 6 Frobenius constants
    uint32_t gamma_live, delta_live; // 0: gamma / delta is at infinity (the pair contributes 1)
    uint32_t gamma_steps, delta_steps;  // lines before the table's running point met a zero slope denominator (MILLER_STEPS: never)
};

// how a field reads the library's 48-byte Montgomery (R = 2^384) form; the bytes are below p (checked by the caller)
template <class F1> struct FieldIn;
template <> struct FieldIn<Fp28Ops> {
    BZK_HD static Fp28 load(const uint8_t* b) {
        Fp a;
#pragma unroll
        for (int i = 0; i < 12; ++i) a.l[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
        return fp28::to28(a);
    }
};
// little-endian bytes of `words` 32-bit words >= mod ?
BZK_HD bool bytes_geq(const uint8_t* b, const uint32_t* mod, int words) {
#pragma unroll 1
    for (int i = words - 1; i >= 0; --i) {
        const uint32_t w = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) | ((uint32_t)b[4 * i + 3] << 24);
        if (w != mod[i]) return w > mod[i];
    }
    return true;
}
template <class F1> BZK_HD bool g1_read(const uint8_t* in, typename F1::T& x, typename F1::T& y) {   // 96 bytes: range and curve
    if (bytes_geq(in, FpParams::MOD, 12) || bytes_geq(in + 48, FpParams::MOD, 12)) return false;
    x = FieldIn<F1>::load(in);
    y = FieldIn<F1>::load(in + 48);
    const typename F1::T four = F1::dbl(F1::dbl(F1::one()));
    return F1::eq(F1::sqr(y), F1::add(F1::mul(F1::sqr(x), x), four));
}
template <class F1, class F2> BZK_HD bool g2_read(const uint8_t* in, typename F2::T& x, typename F2::T& y) {   // 192 bytes
    for (int k = 0; k < 4; ++k)
        if (bytes_geq(in + 48 * k, FpParams::MOD, 12)) return false;
    x = {FieldIn<F1>::load(in), FieldIn<F1>::load(in + 48)};
    y = {FieldIn<F1>::load(in + 96), FieldIn<F1>::load(in + 144)};
    const typename F1::T four = F1::dbl(F1::dbl(F1::one()));
    const typename F2::T b = {four, four};
    return F2::eq(F2::sqr(y), F2::add(F2::mul(F2::sqr(x), x), b));
}

// ---- step 1: the checks of one proof and X = IC_0 + sum x_i IC_i.  Leaves A, X, C, B in their slots and returns the FLAG_* word: FLAG_REFUSED
// (a coordinate not below p, a point off its curve, an input not below r: the verdict is 0) or which pairs are live (both members finite).
// The scalars share their doublings (4-bit windows, most significant first), every addition is a mixed one against the key's affine table;
// X is made affine with one inversion.  sc: 8 n_inputs words of this proof's own (the canonical scalars), word j at sc[j * sc_stride]: word-major
// on the device like the slab (a wavefront's read of one word is one row), contiguous on the host.
template <class L>
BZK_HD uint32_t prepare_one(const L& l, const KeyView<typename L::F1, typename L::F2>& k, const uint8_t* inputs, const uint8_t* proof, uint32_t* sc,
                            uint32_t sc_stride) {
    typedef typename L::F1 F1;
    typedef typename L::F2 F2;
    typedef typename F1::T E1;
    uint32_t flags = 0;
    const bool a_inf = proof[96] != 0, b_inf = proof[289] != 0, c_inf = proof[386] != 0;
    E1 x, y;
    if (!a_inf) {
        if (!g1_read<F1>(proof, x, y)) return FLAG_REFUSED;
        l.st1(slot::PA, x); l.st1(slot::PA + 1, y);
    }
    if (!b_inf) {
        typename F2::T bx, by;
        if (!g2_read<F1, F2>(proof + 97, bx, by)) return FLAG_REFUSED;
        st2(l, slot::QB, bx); st2(l, slot::QB + 2, by);
    }
    if (!c_inf) {
        if (!g1_read<F1>(proof + 290, x, y)) return FLAG_REFUSED;
        l.st1(slot::PC, x); l.st1(slot::PC + 1, y);
    }
    if (!a_inf && !b_inf) flags |= FLAG_AB;
    if (!c_inf) flags |= FLAG_C;
#pragma unroll 1
    for (uint32_t i = 0; i < k.n_inputs; ++i) {
        if (bytes_geq(inputs + 32 * i, FrParams::MOD, 8)) return FLAG_REFUSED;
        Fr s;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const uint8_t* b = inputs + 32 * i + 4 * w;
            s.l[w] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
        s = fe_from_mont<FrParams>(s);
#pragma unroll
        for (int w = 0; w < 8; ++w) sc[(size_t)(8 * i + w) * sc_stride] = s.l[w];
    }
    XyzzT<F1> r = xyzz_identity<F1>();
#pragma unroll 1
    for (int nib = 63; nib >= 0; --nib) {
        if (nib != 63) {
#pragma unroll 1
            for (int d = 0; d < 4; ++d) r = xyzz_dbl<F1>(r);
        }
#pragma unroll 1
        for (uint32_t i = 0; i < k.n_inputs; ++i) {
            const uint32_t w = (sc[(size_t)(8 * i + (nib >> 3)) * sc_stride] >> ((nib & 7) * 4)) & 15u;
            if (!w) continue;
            const uint32_t e = 15 * i + w - 1;
            if (k.tab_inf[e]) continue;
            const AffineT<F1> q = {k.tab_xy[2 * e], k.tab_xy[2 * e + 1]};
            xyzz_add_mixed<F1>(r, q);
        }
    }
    {
        const uint32_t e = 15 * k.n_inputs;
        if (!k.tab_inf[e]) {
            const AffineT<F1> q = {k.tab_xy[2 * e], k.tab_xy[2 * e + 1]};
            xyzz_add_mixed<F1>(r, q);
        }
    }
    AffineT<F1> xa;
    if (xyzz_to_affine<F1>(r, xa)) {
        flags |= FLAG_X;
        l.st1(slot::PX, xa.x); l.st1(slot::PX + 1, xa.y);
    }
    return flags;
}

// ---- step 2: f(A, B) f(X, -gamma) f(C, -delta) m in slot F: the shared accumulator over the 63 steps, the (A, B) pair with its own running point,
// the two fixed pairs from the key's line tables.  Returns flags, with FLAG_DEGENERATE when a live pair met a zero slope denominator (the verdict
// is then 0 and F holds nothing).
template <class L>
BZK_HD uint32_t miller_one(const L& l, const KeyView<typename L::F1, typename L::F2>& k, uint32_t flags) {
    using namespace slot;
    typedef typename L::F1 F1;
    const bool ab = (flags & FLAG_AB) != 0, gx = (flags & FLAG_X) && k.gamma_live, dc = (flags & FLAG_C) && k.delta_live;
    if ((gx && k.gamma_steps < (uint32_t)MILLER_STEPS) || (dc && k.delta_steps < (uint32_t)MILLER_STEPS)) return flags | FLAG_DEGENERATE;
    e12_set_one(l, F);
    if (ab) {
#pragma unroll 1
        for (int i = 0; i < 4; ++i) l.st1(TT + i, l.ld1(QB + i));   // X, Y of B ...
        l.st1(TT + 4, F1::one());                                    // ... and Z = 1
        l.st1(TT + 5, F1::zero());
    }
    int step = 0;
#pragma unroll 1
    for (int i = 62; i >= 0; --i) {
        const int adds = (int)((X_ABS >> i) & 1);
#pragma unroll 1
        for (int s = 0; s <= adds; ++s, ++step) {
            if (s == 0) e12_sqr(l, F, F, TMP);
            if (ab) {
                if (!(s == 0 ? s_dbl_step(l, TT, PA, LINE) : s_add_step(l, TT, QB, PA, LINE))) return flags | FLAG_DEGENERATE;
                e12_mul_by_014(l, F, LINE, TMP);
            }
            if (gx) {
                s_fixed_line(l, LINE, k.gamma + 3 * step, PX);
                e12_mul_by_014(l, F, LINE, TMP);
            }
            if (dc) {
                s_fixed_line(l, LINE, k.delta + 3 * step, PC);
                e12_mul_by_014(l, F, LINE, TMP);
            }
        }
    }
    e12_conj(l, F, F);   // the curve parameter is -|x|
#pragma unroll 1
    for (int i = 0; i < 12; ++i) l.st1(R4 + i, k.m[i]);
    e12_mul(l, F, F, R4, TMP);
    return flags;
}

// ---- step 3: is (the value in slot F)^((p^12 - 1) / r) one ?
template <class L>
BZK_HD bool finalexp_one(const L& l, const KeyView<typename L::F1, typename L::F2>& k) {
    final_exp(l, k.frob);
    return e12_is_one(l, slot::R4);
}

#undef BZK_TW

}  // namespace pairing
}  // namespace bzk
