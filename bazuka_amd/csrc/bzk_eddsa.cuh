// Jubjub EdDSA verification, one signature per lane (eddsa.hip jubjub_verify_kernel; the CPU harness tests/host/eddsa_check.hip runs the same code):
//     ok = pk on curve  and  R on curve  and  h pk + R == s BASE,   h = Poseidon(R.x, R.y, pk.x, pk.y, msg)
// the reference's `JubJub::verify` (src/crypto/jubjub/mod.rs:151-167).  The unified addition law is complete on Jubjub (d is a non-square, a = -1 a
// square), so the verdict is the plain group equation, checked without an inversion:  T = s BASE - h pk  against R projectively.
//
//   h, s        the full integers below r (`to_le_bits`), NOT reduced modulo the subgroup order: pk and R may lie outside the subgroup
//   - h pk      signed radix-8 digits (Booth, |digit| <= 4, 86 windows over 258 bits) against the lane's own table {1, 2, 3, 4} pk, projective, in
//               LDS on the device (word k of the lane at tab[k * stride]): 3 doublings + one complete projective addition per window.  The digit
//               selects the addend - magnitude from the table, sign by negating X, zero = the identity (0 : 1 : 1) - so every lane runs one stream
//   + s BASE    unsigned radix-16 digits against a table j 16^i BASE (i < 64, j < 16; j = 0 is the identity), affine, the same for every lane: built
//               once per context into global memory (base_table_build); no doublings, one mixed addition per window
//
// Field products per signature (squares counted as products; hash and conversions apart):
//   table {2, 3, 4} pk        2 dbl + 1 add                 2 x 7 + 12           26
//   - h pk                    86 x (3 dbl + add)            86 x (21 + 12)    2 838
//   + s BASE                  64 x mixed add                64 x 11             704
//   curve checks, final test  2 x 4 + 2, conversions 8                           18      total 3 586   (binary joint ladder: 256 x (7 + 11) = 4 608)
//   Poseidon, arity 5         8 full rounds x (18 + 36) + 57 partial x 14 + 25 tail + 6 conversions, about 1 260
#pragma once
#include <vector>

#include "bzk_witfill.cuh"

namespace bzk {
namespace eddsa {

constexpr int VW = 3, VWIN = 86, VTAB = 4;    // variable base: window bits, windows, table entries
constexpr int FW = 4, FWIN = 64, FTAB = 16;   // fixed base
constexpr int TAB_WORDS = VTAB * 3 * fr29::N; // per-lane table: VTAB x (X, Y, Z) x 9 limbs
constexpr size_t BASE_TAB_LEN = (size_t)FWIN * FTAB * 2 + 1;  // (x, y) per entry, then Jubjub's d

// Montgomery-256 limbs of Jubjub's d and of BASE (src/crypto/jubjub/mod.rs:25-45)
constexpr uint32_t D_LIMBS[8] = {0xb974f6b0u, 0x2a522455u, 0x0d9acab3u, 0xfc6cc9efu, 0xc27628d1u, 0x7a08fb94u, 0xfe0e262eu, 0x57f8f6a8u};
constexpr uint32_t BASE_X_LIMBS[8] = {0x547c71aau, 0xc8cd898cu, 0xb3564650u, 0x1e77bad0u, 0x49031ebeu, 0x0b5183a6u, 0xa3031a2cu, 0x4f54a483u};
constexpr uint32_t BASE_Y_LIMBS[8] = {0xffffffd9u, 0x00000026u, 0x003ffc27u, 0x3e1c038bu, 0x88581730u, 0x323016c6u, 0xa901ea00u, 0x56cb8254u};

#if defined(__HIP_DEVICE_COMPILE__)
#define BZK_EDDSA_OPAQUE(p) __asm__ volatile("" : "+v"(p))
#else
#define BZK_EDDSA_OPAQUE(p) __asm__ volatile("" : "+r"(p))
#endif
using wf::fr_sel;

// the limbs of a residue: value < r (`from_repr` refuses anything else)
BZK_HD bool canonical(const Fr& a) {
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) borrow = (((uint64_t)a.l[i] - FrParams::MOD[i] - borrow) >> 63) & 1;
    return borrow != 0;
}
BZK_HD Fr29 f29_sel(bool c, const Fr29& a, const Fr29& b) {
    Fr29 r;
#pragma unroll
    for (int i = 0; i < fr29::N; ++i) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
// a == b mod r for normalised a, b with k <= 35
BZK_HD bool f29_eq(const Fr29& a, const Fr29& b) { return fr29::from29(a).equals(fr29::from29(b)); }

// add-2008-bbjlp, a = -1 (host_zk.hip Proj::add_assign), both operands projective.  p: k 2 (products).  q: Y, Z k 2, X k <= 5 (a negated table entry)
BZK_HD wf::JP jp_add(const wf::JP& p, const wf::JP& q, const Fr29& dc) {
    const Fr29 a = fr29::mul(p.Z, q.Z), b = fr29::sqr(a);
    const Fr29 c = fr29::mul(p.X, q.X), d = fr29::mul(p.Y, q.Y);                      // ka kb = 10, 4
    const Fr29 e = fr29::mul(fr29::mul(dc, c), d);
    const Fr29 f = fr29::sub3(b, e);                                                   // k 5
    const Fr29 g = fr29::norm(fr29::add(b, e));                                        // k 4
    const Fr29 u = fr29::sub3(fr29::sub3(fr29::mul(fr29::add(p.X, p.Y), fr29::add(q.X, q.Y)), c), d);  // 4 x 7 = 28 ; X1 Y2 + Y1 X2   k 8
    return {fr29::mul(fr29::mul(a, f), u), fr29::mul(fr29::mul(a, g), fr29::add(d, c)), fr29::mul(f, g)};  // 10, 16 ; 8, 8 ; 20
}
// PointAffine::is_on_curve: y^2 - x^2 == 1 + d x^2 y^2  (x, y: k 2)
BZK_HD bool on_curve(const Fr29& x, const Fr29& y, const Fr29& dc) {
    const Fr29 xx = fr29::sqr(x), yy = fr29::sqr(y);
    const Fr29 lhs = fr29::sub3(yy, xx);                                                                   // k 5
    const Fr29 rhs = fr29::norm(fr29::add(fr29::from_consts(fr29::ONE), fr29::mul(dc, fr29::mul(xx, yy)))); // k 3
    return f29_eq(lhs, rhs);
}

BZK_HD void tab_store(uint32_t* tab, size_t stride, int e, const wf::JP& p) {
    uint32_t* t = tab + (size_t)(e * 3 * fr29::N) * stride;
#pragma unroll
    for (int i = 0; i < fr29::N; ++i) {
        t[(size_t)i * stride] = p.X.l[i];
        t[(size_t)(fr29::N + i) * stride] = p.Y.l[i];
        t[(size_t)(2 * fr29::N + i) * stride] = p.Z.l[i];
    }
}
BZK_HD wf::JP tab_load(const uint32_t* tab, size_t stride, uint32_t e) {  // e < VTAB: a run-time index into the lane's LDS column, not into registers
    const uint32_t* t = tab + (size_t)(e * 3 * fr29::N) * stride;
    wf::JP p;
#pragma unroll
    for (int i = 0; i < fr29::N; ++i) {
        p.X.l[i] = t[(size_t)i * stride];
        p.Y.l[i] = t[(size_t)(fr29::N + i) * stride];
        p.Z.l[i] = t[(size_t)(2 * fr29::N + i) * stride];
    }
    return p;
}

// One signature.  pub = x | y, sig = r.x | r.y | s (Montgomery-256 limbs); pconsts: the sparse Poseidon constants of width 6 (bzk_poseidon29.cuh);
// base_tab: base_table_build's output; tab / stride: TAB_WORDS words of the lane's own.  A field that is not the limbs of a residue gives 0.
BZK_HD uint8_t verify_one(const Fr* __restrict__ pub, const Fr* __restrict__ msg, const Fr* __restrict__ sig, const Fr29* __restrict__ pconsts, int rf,
                          int rp, const Fr29* __restrict__ base_tab, uint32_t* tab, size_t stride) {
    Fr in[5] = {sig[0], sig[1], pub[0], pub[1], msg[0]};
    bool ok = canonical(sig[2]);
#pragma unroll
    for (int i = 0; i < 5; ++i) ok = ok && canonical(in[i]);
    const bool residues = ok;
    if (!residues) {  // the arithmetic below is only bounded for residues: run it on zeros (pk = (0, 0) is off the curve), the verdict is 0
#pragma unroll
        for (int i = 0; i < 5; ++i) in[i] = Fr::zero();
    }
    const Fr29 dc = base_tab[BASE_TAB_LEN - 1], one = fr29::from_consts(fr29::ONE), zero = fr29::zero();
    Fr hc;
    {
        const Fr29 x = fr29::to29(in[2]), y = fr29::to29(in[3]);
        ok = ok && on_curve(x, y, dc) && on_curve(fr29::to29(in[0]), fr29::to29(in[1]), dc);
        const wf::JP p1 = {x, y, one}, p2 = wf::jp_dbl(p1);
        tab_store(tab, stride, 0, p1);
        tab_store(tab, stride, 1, p2);
        tab_store(tab, stride, 2, jp_add(p2, p1, dc));
        tab_store(tab, stride, 3, wf::jp_dbl(p2));
        hc = fe_from_mont<FrParams>(poseidon29_hash<6>(in, pconsts, rf, rp));
    }
    // ---- - h pk.  v = hc << 30 in 9 words: bit 257 of hc (0: hc < 2^255) is the top bit, so the top four bits are window 85's b_257 .. b_254; each
    // window then shifts by three.  Digit of bits b3 b2 b1 b0 (b0 = the bit below the window): 2 b2 + b1 + b0 - 4 b3 (the sum over the windows
    // telescopes to hc - 2^258 b_257 = hc)
    uint32_t v[9];
    v[0] = hc.l[0] << 30;
#pragma unroll
    for (int i = 1; i < 8; ++i) v[i] = (hc.l[i] << 30) | (hc.l[i - 1] >> 2);
    v[8] = hc.l[7] >> 2;
    wf::JP acc = {zero, one, one};
#pragma unroll 1
    for (int w = 0; w < VWIN; ++w) {
        const uint32_t b = v[8] >> 28;
        const int dgt = (int)(b >> 1) + (int)(b & 1u) - (int)((b >> 3) << 3);  // [-4, 4]
#pragma unroll
        for (int i = 8; i > 0; --i) v[i] = (v[i] << VW) | (v[i - 1] >> (32 - VW));
        v[0] <<= VW;
        const uint32_t mag = (uint32_t)(dgt < 0 ? -dgt : dgt);
        wf::JP q = tab_load(tab, stride, mag ? mag - 1u : 0u);
        q.X = f29_sel(dgt > 0, fr29::sub3(zero, q.X), q.X);  // the addend is -dgt pk: k 5 when negated
        q = wf::jp_sel(mag != 0, q, wf::JP{zero, one, one});
        acc = wf::jp_dbl(wf::jp_dbl(wf::jp_dbl(acc)));
        acc = jp_add(acc, q, dc);
    }
    // ---- + s BASE: window i of sc (< 2^255: 64 nibbles) picks j 16^i BASE.  s and R are read again here, through a pointer the compiler cannot
    // see through, instead of being carried in 24 registers across the loop above
    BZK_EDDSA_OPAQUE(sig);
    Fr sc = fe_from_mont<FrParams>(fr_sel(residues, sig[2], Fr::zero()));
#pragma unroll 1
    for (int w = 0; w < FWIN; ++w) {
        const Fr29* e = base_tab + ((size_t)w * FTAB + (sc.l[0] & (FTAB - 1u))) * 2;
#pragma unroll
        for (int i = 0; i < 7; ++i) sc.l[i] = (sc.l[i] >> FW) | (sc.l[i + 1] << (32 - FW));
        sc.l[7] >>= FW;
        acc = wf::jp_add_affine(acc, e[0], e[1], dc);
    }
    // ---- T == R: T.X == R.x T.Z and T.Y == R.y T.Z (T.Z != 0 on the curve)
    const Fr29 rx = fr29::to29(fr_sel(residues, sig[0], Fr::zero())), ry = fr29::to29(fr_sel(residues, sig[1], Fr::zero()));
    ok = ok && f29_eq(acc.X, fr29::mul(rx, acc.Z)) && f29_eq(acc.Y, fr29::mul(ry, acc.Z));
    return ok ? 1 : 0;
}

// The fixed-base table, host side (plain C++ over the same field code): entry (i, j) = j 16^i BASE as affine (x, y) in the 29-bit form, then d.
// 1 024 points, one Fermat inversion each: a few milliseconds, once per context.
inline void base_table_build(std::vector<Fr29>& out) {
    Fr dF, bxF, byF;
    for (int i = 0; i < 8; ++i) { dF.l[i] = D_LIMBS[i]; bxF.l[i] = BASE_X_LIMBS[i]; byF.l[i] = BASE_Y_LIMBS[i]; }
    const Fr29 dc = fr29::to29(dF), one = fr29::from_consts(fr29::ONE), zero = fr29::zero();
    auto affine = [&](const wf::JP& p, Fr29& x, Fr29& y) {
        const Fr29 zi = fr29::inv(p.Z);
        x = fr29::mul(p.X, zi);
        y = fr29::mul(p.Y, zi);
    };
    out.assign(BASE_TAB_LEN, zero);
    Fr29 bx = fr29::to29(bxF), by = fr29::to29(byF);
    for (int i = 0; i < FWIN; ++i) {
        Fr29* row = out.data() + (size_t)i * FTAB * 2;
        row[0] = zero; row[1] = one;
        row[2] = bx; row[3] = by;
        for (int j = 2; j < FTAB; ++j) affine(wf::jp_add_affine(wf::JP{row[2 * j - 2], row[2 * j - 1], one}, bx, by, dc), row[2 * j], row[2 * j + 1]);
        wf::JP p = {bx, by, one};
        for (int k = 0; k < FW; ++k) p = wf::jp_dbl(p);
        affine(p, bx, by);
    }
    out[BASE_TAB_LEN - 1] = dc;
}

}  // namespace eddsa
}  // namespace bzk
