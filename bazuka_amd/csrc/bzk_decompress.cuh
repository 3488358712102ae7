// Jubjub key decompression, one key per lane (eddsa.hip jubjub_decompress_kernel; the CPU harness tests/host/decompress_check.hip runs the same code):
//     y = sqrt((1 + x^2) / (1 - d x^2)), negated when the parity of its canonical integer differs from `odd`
// the reference's `PointCompressed::decompress` (src/crypto/jubjub/curve.rs:78-88).  1 - d x^2 is never zero (d is a non-square).
//
// Fr has 2-adicity 32: r - 1 = 2^32 t, t odd, and g = 7^t generates the subgroup of order 2^32.  The inversion and the square root are ONE
// exponentiation: with u = 1 + x^2, v = 1 - d x^2 and A = u v (the same quadratic character as u / v) the lane computes X = A^(-1/2) and
// y = u X, so y^2 = u^2 / (u v) = u / v.  Tonelli-Shanks on a = 1 / A needs a^((t+1)/2) and a^t; both come from w = A^((t-1)/2):
//     A^t = w^2 A,   a^t = A^(-t) = (A^t)^(2^32 - 1)   (A^(2^32 t) = 1),   a^((t+1)/2) = A^(-t) w
// Every lane of a wave runs one instruction stream: the exponents are constants, and the 2^32-part is removed bit by bit with fixed trip counts
// and selects.  Invariant of round i (0 .. 30): x^2 = a b, the order of b divides 2^(31-i), z has order 2^(32-i).  c = b^(2^(30-i)) is 1 or -1;
// where it is -1, x *= z and b *= z^2; then z = z^2.  After round 30 b = 1 for a residue.  A non-residue leaves some x: the caller's check
// y^2 v == u then fails, which is how it is reported.  A = 0 (u = 0: x^2 = -1) gives X = 0, y = 0, and the check holds: y = 0 is accepted.
//
// Field products per key (squares counted as products; a separate inversion + square root: 417 + 945):
//   x into the 29-bit form, x^2, d x^2, u v                                          4
//   w = A^((t-1)/2)                  221 squares + 131 products                     352
//   A^t, A^(-t), a^((t+1)/2)         2 + (31 squares + 5 products) + 1               39
//   31 rounds                        465 squares of c + 31 x (test, x z, z^2, b z^2) 589
//   y = u X, y^2 v == u (2 + 2 conversions), y out, parity                            7      total 991
#pragma once
#include "bzk_eddsa.cuh"

namespace bzk {
namespace eddsa {

// 2^261 d and 2^261 7^t mod r in 29-bit limbs
constexpr fr29::Consts D29 = {{0x0e9ed5e8u, 0x12245679u, 0x002d9f52u, 0x03bb3367u, 0x0d9bfb3du, 0x18ebb3ccu, 0x1c29ceccu, 0x0a7b6020u, 0x0020d725u}};
constexpr fr29::Consts G29 = {{0x01c8cd27u, 0x158d8d27u, 0x19006c0du, 0x09177006u, 0x1b40635eu, 0x01d0b1cau, 0x0d517805u, 0x04859aa2u, 0x002c4064u}};

BZK_HD Fr29 f29_sqr_n(Fr29 x, int n) {
#pragma unroll 1
    for (int i = 0; i < n; ++i) x = fr29::sqr(x);
    return x;
}
BZK_HD bool f29_is_one(const Fr29& a) { return fr29::from29(a).equals(Fr::one()); }

// X with X^2 A = 1 for a non-zero residue A; 0 for A = 0; some value otherwise.  Any normalised A with k <= 35; result k 2.
BZK_HD Fr29 f29_isqrt(const Fr29& A) {
    constexpr uint32_t E[7] = {0x7fffffffu, 0x7fff2dffu, 0xa9ded201u, 0x04d0ec02u, 0x199cec04u, 0x94cebea4u, 0x39f6d3a9u};  // (t - 1) / 2, 222 bits
    const Fr29 a = fr29::mul(A, fr29::from_consts(fr29::ONE));  // k 2 whatever A's k
    Fr29 w = a;                                                 // bit 221 (word 6, bit 29) is the top bit
#pragma unroll
    for (int i = 6; i >= 0; --i) {  // unrolled over the words: each word is a constant, nothing is indexed at run time
        const uint32_t e = E[i];
#pragma unroll 1
        for (int j = i == 6 ? 28 : 31; j >= 0; --j) {
            w = fr29::sqr(w);
            if ((e >> j) & 1u) w = fr29::mul(w, a);
        }
    }
    Fr29 b = fr29::mul(fr29::sqr(w), a);  // A^t; then A^(-t) = b^(2^32 - 1) by doubling the run of ones: 2, 4, 8, 16, 32
#pragma unroll 1
    for (int k = 1; k < 32; k <<= 1) b = fr29::mul(f29_sqr_n(b, k), b);
    Fr29 x = fr29::mul(b, w), z = fr29::from_consts(G29);
#pragma unroll 1
    for (int i = 0; i < 31; ++i) {
        const bool minus = !f29_is_one(f29_sqr_n(b, 30 - i));
        x = f29_sel(minus, fr29::mul(x, z), x);
        z = fr29::sqr(z);
        b = f29_sel(minus, fr29::mul(b, z), b);
    }
    return x;
}

// a square root of a (k <= 35, normalised), k 2; *ok: a is a residue (0 is: its root is 0)
BZK_HD Fr29 f29_sqrt(const Fr29& a, bool* ok) {
    const Fr29 s = fr29::mul(a, f29_isqrt(a));
    *ok = f29_eq(fr29::sqr(s), a);
    return s;
}

// One key.  x: Montgomery-256 limbs, odd: the wanted parity of y.  out = x | y and 1, or zeros and 0 where the reference panics (no square
// root) or x is not the limbs of a residue (the lane then runs on zeros, as verify_one does, so that the field's bounds hold for any input).
BZK_HD uint8_t decompress_one(const Fr& x_in, bool odd, Fr* __restrict__ out) {
    const bool residue = canonical(x_in);
    const Fr xm = fr_sel(residue, x_in, Fr::zero());
    const Fr29 one = fr29::from_consts(fr29::ONE);
    const Fr29 xx = fr29::sqr(fr29::to29(xm));
    const Fr29 u = fr29::norm(fr29::add(one, xx));                               // k 3
    const Fr29 v = fr29::sub3(one, fr29::mul(fr29::from_consts(D29), xx));       // k 4
    const Fr29 y = fr29::mul(u, f29_isqrt(fr29::mul(u, v)));
    const bool ok = residue && f29_eq(fr29::mul(fr29::sqr(y), v), u);
    Fr yc = fr29::from29(y);                                                      // canonical Montgomery-256 limbs
    const bool is_odd = (fe_from_mont<FrParams>(yc).l[0] & 1u) != 0;              // parity of the canonical INTEGER
    yc = fr_sel(is_odd != odd, fe_neg<FrParams>(yc), yc);                         // -0 = 0: y = 0 serves either parity
    out[0] = fr_sel(ok, xm, Fr::zero());
    out[1] = fr_sel(ok, yc, Fr::zero());
    return ok ? 1 : 0;
}

// The hash input of one MpnTransaction (src/zk/mod.rs:616-627): nonce, dst.x, dst.y, amount.token, amount, fee.token, fee.  nums = nonce,
// amount, fee as integers: their Montgomery form is made here, one product each (fe_to_mont), not on the host.  tok = the two token ids as
// scalars.  Returns whether the record can verify at all: dst decompressed and the token ids are residues' limbs; zeros are hashed otherwise.
BZK_HD bool tx_tuple_one(const uint64_t* __restrict__ nums, const Fr* __restrict__ tok, const Fr* __restrict__ dst_xy, uint8_t dst_ok,
                         Fr* __restrict__ out) {
    const bool ok = dst_ok != 0 && canonical(tok[0]) && canonical(tok[1]);
    Fr n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Fr c = Fr::zero();
        c.l[0] = (uint32_t)nums[k];
        c.l[1] = (uint32_t)(nums[k] >> 32);
        n[k] = fe_to_mont<FrParams>(c);
    }
    const Fr z = Fr::zero();
    out[0] = fr_sel(ok, n[0], z);
    out[1] = fr_sel(ok, dst_xy[0], z);
    out[2] = fr_sel(ok, dst_xy[1], z);
    out[3] = fr_sel(ok, tok[0], z);
    out[4] = fr_sel(ok, n[1], z);
    out[5] = fr_sel(ok, tok[1], z);
    out[6] = fr_sel(ok, n[2], z);
    return ok;
}

}  // namespace eddsa
}  // namespace bzk
