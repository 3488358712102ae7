// The optimal ate pairing of BLS12-381 on the host, for `groth16_verify` (row a8, host_pairing.hip) and for the CPU harness that checks
// it piece by piece (tests/host/hostcheck.hip).  Plain C++ over the 64-bit-limb host field (host_fp64.h): nothing here runs on the GPU.
//
//   tower    Fp2 = Fp[u] / (u^2 + 1),  Fp6 = Fp2[v] / (v^3 - xi),  xi = 1 + u,  Fp12 = Fp6[w] / (w^2 - v)        (w^6 = xi)
//   Miller   optimal ate over |x| = 0xd201000000010000 (x < 0: conjugate at the end), M-type twist; all pairs share one accumulator (one
//            squaring per step); running points in Jacobian coordinates, lines scaled by their slope's denominator (no inversion at all);
//            a line has three non-zero Fp2 coefficients and is multiplied in as such.  `multi_miller_affine` (slopes of a step inverted
//            together) is the previous form, kept as the yardstick: both loops give the same pairing
//   final    f^((p^12 - 1) / r) up to the cube: easy part (p^6 - 1)(p^2 + 1) by conjugate / inverse / Frobenius, hard part through
//                3 (p^4 - p^2 + 1) / r = (x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3            (integer identity, checked in the tests)
//            i.e. five exponentiations by |x| (63 Granger-Scott squarings + 5 products each, valid in the cyclotomic subgroup the easy part
//            lands in) and two Frobenius maps.  The cube does not matter to a verifier: the target group has prime order r, 3 does not
//            divide r, so g^3 = 1 iff g = 1.  `final_exp_plain` is the 2030-bit square-and-multiply of the first version (round 2): the
//            yardstick of the tests, which check fast == plain^3 on Miller outputs.
// Cost on one core of the build container (Xeon @ 2.1 GHz, -O3): the four-pair check of a Groth16 verification ~2.2 ms (Miller loop ~1.5, final
// exponentiation ~0.6) of the verifier's 2.8 ms; the first version spent 6.8 ms on line inversions and 11 ms on the plain exponentiation.
// Those figures were taken when the tower was plain value code in this file; multi_miller and final_exp now run the shared slot functions of
// bzk_pairing28.cuh on a local slab and have not been re-timed piece by piece (the flagship benchmark, which ends in this verifier, is unchanged).
#pragma once
#include <vector>

#include "host_fp64.h"
#include "bzk_pairing28.cuh"

namespace bzk {
namespace pairing {
template <> struct FieldIn<HFpOps> {
    static HFp load(const uint8_t* b) { HFp r; memcpy(r.l, b, 48); return r; }   // same Montgomery value, same little-endian bytes
};
}  // namespace pairing
namespace hp {

// The tower itself is bzk_pairing28.cuh, generic over the field: Fp2 / Fp6 on values (TW), Fp12 on the slots of a slab.  The functions below are
// its instantiation over the host field with the value signatures the verifier and the CPU harness use: an Fp12 function copies its operands
// into a local slab, runs the slot function and copies the result out.  Those copies are for the harness's piecewise checks only: the loops that
// matter, multi_miller and final_exp, keep their accumulator in one slab from start to end.
typedef HFpOps F1;
typedef HFp2Ops F2;
typedef HFp2 E2;
typedef pairing::Tower<HFpOps, HFp2Ops> TW;
typedef TW::E6 E6;
typedef TW::E12 E12;
struct LaneH {   // the host lane: slot i is s[i]
    typedef HFpOps F1;
    typedef HFp2Ops F2;
    HFp* s;
    HFp ld1(int i) const { return s[i]; }
    void st1(int i, const HFp& v) const { s[i] = v; }
};
static_assert(sizeof(E12) == 12 * sizeof(HFp), "an Fp12 value is twelve slots in tower order");
inline void put12(HFp* s, int at, const E12& a) { memcpy(s + at, &a, sizeof a); }
inline E12 get12(const HFp* s, int at) { E12 r; memcpy(&r, s + at, sizeof r); return r; }

inline HFp to_h(const Fp& a) { HFp r; memcpy(r.l, a.l, 48); return r; }          // same Montgomery value, same little-endian bytes
inline E2 to_h(const Fp2& a) { return {to_h(a.c0), to_h(a.c1)}; }

inline E2 e2_mul_xi(const E2& a) { return TW::e2_mul_xi(a); }
inline E2 e2_scale(const E2& a, const HFp& k) { return TW::e2_scale(a, k); }
inline E2 e2_conj(const E2& a) { return TW::e2_conj(a); }
inline E6 e6_zero() { return TW::e6_zero(); }
inline E6 e6_one() { return TW::e6_one(); }
inline E6 e6_add(const E6& a, const E6& b) { return TW::e6_add(a, b); }
inline E6 e6_sub(const E6& a, const E6& b) { return TW::e6_sub(a, b); }
inline E6 e6_neg(const E6& a) { return TW::e6_neg(a); }
inline E6 e6_mul(const E6& a, const E6& b) { return TW::e6_mul(a, b); }
inline E6 e6_mul_v(const E6& a) { return TW::e6_mul_v(a); }
inline E6 e6_mul_by_01(const E6& a, const E2& b0, const E2& b1) { return TW::e6_mul_by_01(a, b0, b1); }
inline E6 e6_mul_by_1_fp(const E6& a, const HFp& k) { return TW::e6_mul_by_1_fp(a, k); }
inline E6 e6_mul_by_1(const E6& a, const E2& b1) { return TW::e6_mul_by_1(a, b1); }
inline E6 e6_inv(const E6& a) { return TW::e6_inv(a); }
inline E12 e12_one() { return {e6_one(), e6_zero()}; }
inline E12 e12_mul(const E12& a, const E12& b) {
    HFp s[48];
    put12(s, 0, a); put12(s, 12, b);
    pairing::e12_mul(LaneH{s}, 24, 0, 12, 36);
    return get12(s, 24);
}
inline E12 e12_sqr(const E12& a) {
    HFp s[36];
    put12(s, 0, a);
    pairing::e12_sqr(LaneH{s}, 12, 0, 24);
    return get12(s, 12);
}
inline E12 e12_conj(const E12& a) { return {a.a0, e6_neg(a.a1)}; }
inline E12 e12_inv(const E12& a) {
    HFp s[36];
    put12(s, 0, a);
    pairing::e12_inv(LaneH{s}, 12, 0, 24);
    return get12(s, 12);
}
inline bool e6_eq(const E6& a, const E6& b) { return TW::e6_eq(a, b); }
inline bool e12_eq(const E12& a, const E12& b) { return e6_eq(a.a0, b.a0) && e6_eq(a.a1, b.a1); }
inline bool e12_is_one(const E12& a) { return e12_eq(a, e12_one()); }

// f * l for a line l = l00 + l01 v + (l11 v) w with l11 in Fp (the affine loop's lines): 6 + 6 + 3 Fp2-size products instead of 18
inline E12 e12_mul_by_line(const E12& f, const E2& l00, const E2& l01, const HFp& l11) {
    const E6 t0 = e6_mul_by_01(f.a0, l00, l01);
    const E6 t1 = e6_mul_by_1_fp(f.a1, l11);
    E12 r;
    r.a0 = e6_add(t0, e6_mul_v(t1));
    const E2 s01 = {F1::add(l01.c0, l11), l01.c1};
    r.a1 = e6_sub(e6_sub(e6_mul_by_01(e6_add(f.a0, f.a1), l00, s01), t0), t1);
    return r;
}
// the same with l11 in Fp2 (the projective lines): positions 0, 1 and 4 of the tower - 6 + 3 + 6 Fp2 products
inline E12 e12_mul_by_014(const E12& f, const E2& c0, const E2& c1, const E2& c4) {
    HFp s[30];
    put12(s, 0, f);
    memcpy(s + 12, &c0, sizeof c0); memcpy(s + 14, &c1, sizeof c1); memcpy(s + 16, &c4, sizeof c4);
    pairing::e12_mul_by_014(LaneH{s}, 0, 12, 18);
    return get12(s, 0);
}

// ---- the library's packed points.  Montgomery limbs of an Fp element are below p: anything else is not a value `Fp([u64; 6])` can legitimately
// hold, and arithmetic on it would leave the verdict to the reduction details of whichever library runs it
struct G1A { HFp x, y; bool inf; };
struct G2A { E2 x, y; bool inf; };
inline bool fp_in_range(const HFp& a) { return !hfp::geq_p(a.l, hfp::consts().p); }
inline HFp fp_four() { return F1::dbl(F1::dbl(F1::one())); }   // Montgomery form of 4
inline bool g1_unpack(const uint8_t* in, G1A& o) {  // packed 97 bytes; range + on-curve check
    o.inf = in[96] != 0;
    memcpy(o.x.l, in, 48);
    memcpy(o.y.l, in + 48, 48);
    if (o.inf) return true;
    if (!fp_in_range(o.x) || !fp_in_range(o.y)) return false;
    return F1::eq(F1::sqr(o.y), F1::add(F1::mul(F1::sqr(o.x), o.x), fp_four()));
}
inline bool g2_unpack(const uint8_t* in, G2A& o) {
    o.inf = in[192] != 0;
    memcpy(o.x.c0.l, in, 48); memcpy(o.x.c1.l, in + 48, 48); memcpy(o.y.c0.l, in + 96, 48); memcpy(o.y.c1.l, in + 144, 48);
    if (o.inf) return true;
    if (!fp_in_range(o.x.c0) || !fp_in_range(o.x.c1) || !fp_in_range(o.y.c0) || !fp_in_range(o.y.c1)) return false;
    const E2 b = {fp_four(), fp_four()};
    return F2::eq(F2::sqr(o.y), F2::add(F2::mul(F2::sqr(o.x), o.x), b));
}

// ---- Frobenius: (sum_i c_i w^i)^p = sum_i conj(c_i) gamma_i w^i,  gamma_i = xi^(i (p - 1) / 6)
struct FrobConsts { E2 g[6]; };
inline E2 e2_pow(const E2& a, const uint64_t* e, int limbs) {
    E2 r = F2::one();
    for (int i = 64 * limbs - 1; i >= 0; --i) {
        r = F2::sqr(r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = F2::mul(r, a);
    }
    return r;
}
inline const FrobConsts& frob_consts() {
    static const FrobConsts c = [] {
        uint64_t e[6];
        memcpy(e, hfp::consts().p, 48);
        e[0] -= 1;  // p - 1 (p is odd)
        unsigned __int128 rem = 0;  // (p - 1) / 6, exact
        for (int i = 5; i >= 0; --i) {
            const unsigned __int128 cur = (rem << 64) | e[i];
            e[i] = (uint64_t)(cur / 6);
            rem = cur % 6;
        }
        FrobConsts k;
        const E2 xi = {F1::one(), F1::one()};
        k.g[0] = F2::one();
        k.g[1] = e2_pow(xi, e, 6);
        for (int i = 2; i < 6; ++i) k.g[i] = F2::mul(k.g[i - 1], k.g[1]);
        return k;
    }();
    return c;
}
inline E12 e12_frob(const E12& f) {
    HFp s[24];
    put12(s, 0, f);
    pairing::e12_frob(LaneH{s}, 12, 0, frob_consts().g);
    return get12(s, 12);
}
// squaring in the cyclotomic subgroup (Granger - Scott, see bzk_pairing28.cuh)
inline void fp4_sqr(const E2& a, const E2& b, E2& o0, E2& o1) { TW::fp4_sqr(a, b, o0, o1); }
inline E12 e12_cyc_sqr(const E12& f) {
    HFp s[12];
    put12(s, 0, f);
    pairing::e12_cyc_sqr(LaneH{s}, 0, 0);
    return get12(s, 0);
}
static constexpr uint64_t X_ABS = pairing::X_ABS;
// g^x for g in the cyclotomic subgroup (x = -|x|: the inverse there is the conjugate)
inline E12 e12_cyc_exp_x(const E12& g) {
    HFp s[36];
    put12(s, 0, g);
    pairing::e12_cyc_exp_x(LaneH{s}, 12, 0, 24);
    return get12(s, 12);
}
inline E12 final_exp_easy(const E12& f) {   // f^(p^6 - 1)(p^2 + 1)
    HFp s[pairing::slot::COUNT];
    put12(s, pairing::slot::F, f);
    pairing::final_exp_easy(LaneH{s}, frob_consts().g);
    return get12(s, pairing::slot::R1);
}
// (easy part)^( (x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3 ) = f^(3 (p^12 - 1) / r)
inline E12 final_exp(const E12& f) {
    HFp s[pairing::slot::COUNT];
    put12(s, pairing::slot::F, f);
    pairing::final_exp(LaneH{s}, frob_consts().g);
    return get12(s, pairing::slot::R4);
}

// the first version's final exponentiation: easy half by conjugate / inverse, everything else as one exponentiation by (p^6 + 1) / r
inline E12 final_exp_plain(const E12& f) {
    static const uint32_t E[64] = {  // (p^6 + 1) / r, little-endian 32-bit words
        0xc0705d6au, 0x8739e1cdu, 0xe0381a16u, 0x09a5256du, 0x61c791e2u, 0x9cf0f70au, 0x7903f76eu, 0x3a09c449u, 0x3890f133u, 0x2d727156u,
        0x6fec7760u, 0x224741b3u, 0x2a12bd40u, 0x338259c2u, 0x778e0de7u, 0x38ee1cd4u, 0x188a20b0u, 0xc3b5ef4bu, 0xe2764d7bu, 0x1d615d49u,
        0xd076117du, 0x816101ddu, 0x7ebe3afcu, 0xf007c01eu, 0x935021c3u, 0x27d7bd90u, 0x57c0b15fu, 0xc3b5e2f5u, 0xc4f82384u, 0x5e886c94u,
        0x11e63f56u, 0xee6a95dbu, 0x4a9c4f6fu, 0x2b822f51u, 0xd21b73dau, 0x12d6a874u, 0xf499dffbu, 0x1304275eu, 0xbcb95d1fu, 0x967878feu,
        0x8b2f2922u, 0x4744497fu, 0xf0841855u, 0x85a2e707u, 0x6c802eecu, 0x9f0c5012u, 0xbd2fa489u, 0xfb46e197u, 0x9bc5f61au, 0x548ce080u,
        0x73beaa8cu, 0xcf56fb15u, 0x763bdf7cu, 0xad7375a3u, 0x179bdeccu, 0xe0ec9031u, 0x3c48c1dau, 0x6579aea8u, 0x64cf5bb3u, 0xdbf85ae6u,
        0x55ca7566u, 0x7b6f235cu, 0x14877503u, 0x000028b3u};
    const E12 g = e12_mul(e12_conj(f), e12_inv(f));
    E12 r = e12_one();
    for (int i = 2029; i >= 0; --i) {
        r = e12_sqr(r);
        if ((E[i >> 5] >> (i & 31)) & 1) r = e12_mul(r, g);
    }
    return r;
}

// ---- Miller loop

// f *= the line through T (twist coordinates, slope lam) evaluated at P, up to a factor the final exponentiation kills:
// (lam xT - yT) + (-lam xP) w^2 + yP w^3
inline E12 mul_line(const E12& f, const E2& lam, const G2A& t, const G1A& p) {
    return e12_mul_by_line(f, F2::sub(F2::mul(lam, t.x), t.y), e2_scale(F2::neg(lam), p.x), p.y);
}
// out[k] = 1 / d[k] for the n <= 4 live denominators; false when one of them is zero
inline bool batch_inv(const E2* d, int n, E2* out) {
    E2 pre[4];
    E2 acc = F2::one();
    for (int k = 0; k < n; ++k) {
        if (F2::is_zero(d[k])) return false;
        pre[k] = acc;
        acc = F2::mul(acc, d[k]);
    }
    E2 inv = F2::inv(acc);
    for (int k = n - 1; k >= 0; --k) {
        out[k] = F2::mul(inv, pre[k]);
        inv = F2::mul(inv, d[k]);
    }
    return true;
}
// product of the Miller functions of n <= 4 pairs (pairs with an identity member contribute 1).  *degenerate is set when a line's slope
// has a zero denominator (T of order 2, or T = +-Q): impossible for points of the prime-order subgroup, reachable only with low-order G2
// points, which the callers only check to be on the curve (as the reference does - it transmutes unchecked points into bellman's
// projective Miller loop).  Such a proof cannot satisfy the pairing equation; the verdict is then "does not verify" instead of a value
// computed from 1 / 0.
// Running points in JACOBIAN coordinates (x = X / Z^2, y = Y / Z^3): no inversion anywhere.  The affine line
//     (lam xT - yT) - lam xP w^2 + yP w^3
// is used multiplied by its slope's denominator (an Fp2 factor the final exponentiation removes):
//   doubling  lam = 3 X^2 / (2 Y Z),          x 2 Y Z^3:   (3 X^3 - 2 Y^2)  -  3 X^2 Z^2 xP w^2  +  2 Y Z^3 yP w^3
//   addition  lam = (yQ Z^3 - Y) / (Z H),     x Z H:       (R xQ - yQ Z H)  -  R xP w^2          +  Z H yP w^3       H = xQ Z^2 - X, R = yQ Z^3 - Y
typedef TW::G2J G2J;
inline E12 multi_miller(const G1A* p, const G2A* q, int n, bool* degenerate) {
    G2J t[4];
    int live[4], nl = 0;
    for (int k = 0; k < n && k < 4; ++k)
        if (!p[k].inf && !q[k].inf) { t[nl] = {q[k].x, q[k].y, F2::one()}; live[nl++] = k; }
    // the accumulator stays in a local slab through the loop: f in slots 0 .. 11, the line in 12 .. 17, temporaries in 18 .. 29
    HFp s[30];
    const LaneH l = {s};
    const auto mul_line014 = [&](const E2& l00, const E2& c1, const E2& c4) {
        pairing::st2(l, 12, l00); pairing::st2(l, 14, c1); pairing::st2(l, 16, c4);
        pairing::e12_mul_by_014(l, 0, 12, 18);
    };
    pairing::e12_set_one(l, 0);
    for (int i = 62; i >= 0; --i) {  // bit 63 is the leading one
        pairing::e12_sqr(l, 0, 0, 18);
        for (int j = 0; j < nl; ++j) {
            G2J& T = t[j];
            const G1A& P = p[live[j]];
            E2 l00, cx, cy;
            if (!TW::dbl_coeffs(T, l00, cx, cy)) { *degenerate = true; return e12_one(); }   // vertical tangent
            mul_line014(l00, e2_scale(cx, P.x), e2_scale(cy, P.y));
        }
        if ((X_ABS >> i) & 1) {
            for (int j = 0; j < nl; ++j) {
                G2J& T = t[j];
                const G1A& P = p[live[j]];
                const G2A& Q = q[live[j]];
                E2 l00, cx, cy;
                if (!TW::add_coeffs(T, Q.x, Q.y, l00, cx, cy)) { *degenerate = true; return e12_one(); }   // T = +-Q
                mul_line014(l00, e2_scale(cx, P.x), e2_scale(cy, P.y));
            }
        }
    }
    return e12_conj(get12(s, 0));  // the curve parameter is -|x|
}

// the same product with AFFINE running points (slopes inverted together, one Fp2 inversion per step): the second version, kept as the
// yardstick of the projective loop - the two differ by Fp2 factors per line, which the final exponentiation removes: equal pairings
inline E12 multi_miller_affine(const G1A* p, const G2A* q, int n, bool* degenerate) {
    G2A t[4];
    int live[4], nl = 0;
    for (int k = 0; k < n && k < 4; ++k)
        if (!p[k].inf && !q[k].inf) { t[nl] = q[k]; live[nl++] = k; }
    E12 f = e12_one();
    E2 den[4], inv[4];
    for (int i = 62; i >= 0; --i) {  // bit 63 is the leading one
        f = e12_sqr(f);
        for (int j = 0; j < nl; ++j) den[j] = F2::add(t[j].y, t[j].y);
        if (!batch_inv(den, nl, inv)) { *degenerate = true; return e12_one(); }
        for (int j = 0; j < nl; ++j) {
            const E2 xx = F2::sqr(t[j].x);
            const E2 lam = F2::mul(F2::add(F2::add(xx, xx), xx), inv[j]);
            f = mul_line(f, lam, t[j], p[live[j]]);
            const E2 x3 = F2::sub(F2::sqr(lam), F2::add(t[j].x, t[j].x));
            t[j] = {x3, F2::sub(F2::mul(lam, F2::sub(t[j].x, x3)), t[j].y), false};
        }
        if ((X_ABS >> i) & 1) {
            for (int j = 0; j < nl; ++j) den[j] = F2::sub(q[live[j]].x, t[j].x);
            if (!batch_inv(den, nl, inv)) { *degenerate = true; return e12_one(); }
            for (int j = 0; j < nl; ++j) {
                const G2A& qq = q[live[j]];
                const E2 lam = F2::mul(F2::sub(qq.y, t[j].y), inv[j]);
                f = mul_line(f, lam, t[j], p[live[j]]);
                const E2 x3 = F2::sub(F2::sub(F2::sqr(lam), t[j].x), qq.x);
                t[j] = {x3, F2::sub(F2::mul(lam, F2::sub(t[j].x, x3)), t[j].y), false};
            }
        }
    }
    return e12_conj(f);  // the curve parameter is -|x|
}

// ==== a verifying key as the batched verifier prepares it, once per call (verify.hip; tests/host/pairing28_check.hip)
// ---- what a call prepares from its key, in the host field
struct KeyHost {
    bool valid = false;   // false: InvalidVerifyingKey, or a key point off its curve / out of range - every verdict is 0
    uint32_t n_inputs = 0;
    std::vector<HFp> tab_xy;
    std::vector<uint8_t> tab_inf;
    std::vector<HFp2> gamma, delta;
    uint32_t gamma_live = 0, delta_live = 0, gamma_steps = 0, delta_steps = 0;
    HFp m[12];
    pairing::KeyView<HFpOps, HFp2Ops> view() const {
        return {n_inputs, tab_xy.data(), tab_inf.data(), gamma.data(), delta.data(), m, frob_consts().g, gamma_live, delta_live, gamma_steps,
                delta_steps};
    }
};
// the line coefficients of the running point of q over the whole loop (they do not depend on the first argument); returns how many lines there
// are before a zero slope denominator (MILLER_STEPS: all of them)
inline uint32_t line_table(const G2A& q, std::vector<HFp2>& out) {
    out.assign((size_t)3 * pairing::MILLER_STEPS, HFp2Ops::zero());
    TW::G2J T = {q.x, q.y, HFp2Ops::one()};
    uint32_t step = 0;
    for (int i = 62; i >= 0; --i) {
        if (!TW::dbl_coeffs(T, out[3 * step], out[3 * step + 1], out[3 * step + 2])) return step;
        ++step;
        if ((pairing::X_ABS >> i) & 1) {
            if (!TW::add_coeffs(T, q.x, q.y, out[3 * step], out[3 * step + 1], out[3 * step + 2])) return step;
            ++step;
        }
    }
    return step;
}
inline void key_prepare(const uint8_t* vk, uint64_t vk_len, uint32_t n_inputs, KeyHost& K) {
    K.n_inputs = n_inputs;
    uint64_t n_ic;
    memcpy(&n_ic, vk + 870, 8);
    if (n_ic != (uint64_t)n_inputs + 1 || vk_len != 878 + 97 * n_ic) return;  // verify_proof: VerificationError::InvalidVerifyingKey
    G1A alpha, ic;
    G2A beta, gamma, delta;
    if (!g1_unpack(vk, alpha) || !g2_unpack(vk + 194, beta) || !g2_unpack(vk + 387, gamma) || !g2_unpack(vk + 677, delta)) return;
    // j IC_i for j = 1 .. 15 (the 4-bit windows of input i), affine, and IC_0 last; an entry may be the identity (IC_i at infinity, or of small order)
    typedef XyzzT<HFpOps> Pt;
    const size_t entries = (size_t)15 * n_inputs + 1;
    K.tab_xy.assign(2 * entries, HFpOps::zero());
    K.tab_inf.assign(entries, 1);
    auto put = [&](size_t e, const Pt& p) {
        AffineT<HFpOps> a;
        if (!xyzz_to_affine<HFpOps>(p, a)) return;
        K.tab_inf[e] = 0;
        K.tab_xy[2 * e] = a.x;
        K.tab_xy[2 * e + 1] = a.y;
    };
    for (uint64_t i = 0; i < n_ic; ++i) {
        if (!g1_unpack(vk + 878 + 97 * i, ic)) return;
        const Pt one = ic.inf ? xyzz_identity<HFpOps>() : xyzz_from_affine<HFpOps>({ic.x, ic.y});
        if (i == 0) {
            put(entries - 1, one);
            continue;
        }
        Pt t = one;
        for (int j = 0; j < 15; ++j) {
            put(15 * (i - 1) + j, t);
            xyzz_add<HFpOps>(t, one);
        }
    }
    // e(A, B) e(X, -gamma) e(C, -delta) e(-alpha, beta) == 1
    gamma.y = F2::neg(gamma.y);
    delta.y = F2::neg(delta.y);
    alpha.y = F1::neg(alpha.y);
    K.gamma_live = !gamma.inf;
    K.delta_live = !delta.inf;
    K.gamma_steps = gamma.inf ? (uint32_t)pairing::MILLER_STEPS : line_table(gamma, K.gamma);
    K.delta_steps = delta.inf ? (uint32_t)pairing::MILLER_STEPS : line_table(delta, K.delta);
    if (gamma.inf) K.gamma.assign((size_t)3 * pairing::MILLER_STEPS, HFp2Ops::zero());
    if (delta.inf) K.delta.assign((size_t)3 * pairing::MILLER_STEPS, HFp2Ops::zero());
    bool degenerate = false;
    const E12 m = multi_miller(&alpha, &beta, 1, &degenerate);   // a constant of the key: Miller functions of a shared accumulator multiply
    if (degenerate) return;                                      // the single call meets the same exit in its loop: 0 whatever the proof
    memcpy(K.m, &m, sizeof m);
    K.valid = true;
}

inline Fp28 h_to28(const HFp& a) {
    Fp t;
    memcpy(t.l, a.l, 48);
    return fp28::to28(t);
}
// the key's tables in the device field, packed into one upload: tab_xy | gamma | delta | m | frob | tab_inf
struct KeyUpload {
    std::vector<uint8_t> bytes;
    size_t at_tab = 0, at_gamma = 0, at_delta = 0, at_m = 0, at_frob = 0, at_inf = 0;
    explicit KeyUpload(const KeyHost& K) {
        std::vector<Fp28> f;
        auto put2 = [&](const HFp2& a) { f.push_back(h_to28(a.c0)); f.push_back(h_to28(a.c1)); };
        at_tab = 0;
        for (const HFp& a : K.tab_xy) f.push_back(h_to28(a));
        at_gamma = f.size() * sizeof(Fp28);
        for (const HFp2& a : K.gamma) put2(a);
        at_delta = f.size() * sizeof(Fp28);
        for (const HFp2& a : K.delta) put2(a);
        at_m = f.size() * sizeof(Fp28);
        for (int i = 0; i < 12; ++i) f.push_back(h_to28(K.m[i]));
        at_frob = f.size() * sizeof(Fp28);
        for (int i = 0; i < 6; ++i) put2(frob_consts().g[i]);
        at_inf = f.size() * sizeof(Fp28);
        bytes.resize(at_inf + K.tab_inf.size());
        memcpy(bytes.data(), f.data(), at_inf);
        memcpy(bytes.data() + at_inf, K.tab_inf.data(), K.tab_inf.size());
    }
    pairing::KeyView<Fp28Ops, Fp2x28Ops> view(const KeyHost& K, const uint8_t* d) const {
        return {K.n_inputs, (const Fp28*)(d + at_tab), d + at_inf, (const Fp2x28*)(d + at_gamma), (const Fp2x28*)(d + at_delta),
                (const Fp28*)(d + at_m), (const Fp2x28*)(d + at_frob), K.gamma_live, K.delta_live, K.gamma_steps, K.delta_steps};
    }
};

}  // namespace hp
}  // namespace bzk
