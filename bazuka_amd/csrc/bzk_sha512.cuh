// SHA-512 (FIPS 180-4), one message per lane (eddsa.hip sha512_kernel and the hash of ed25519_verify_kernel; the CPU harness
// tests/host/ed25519_check.hip and the ctx = NULL entries run the same code).
//
// The eight state words and the sixteen-word schedule ring are 64-bit values that every access names with a constant index: the sixteen rounds of
// one trip round the ring are unrolled, the five trips are a rolled loop whose round constants are uniform loads.  Sixteen rounds are two turns of
// the a .. h rotation, so the names are back in place at the end of a trip.  The 64-bit rotations are written on the 32-bit halves (one funnel
// shift per half: v_alignbit_b32), as bzk_keccak.cuh's are.
//
// A message is up to three byte ranges and an optional literal last byte, hashed in that order without a copy: Ed25519 hashes R | A | M, and
// the signed form of a ContractDeposit is its bytes up to the Option<Signature> tag followed by a None tag (src/core/transaction.rs:192-202).
// Bytes are fetched eight at a time where the word lies inside one range, byte by byte at range edges, the tail and the padding.
//
// sha512_one is a template on the message type: the same rounds absorb a gathered message (bzk_gather.cuh: up to six pieces, each a range or a
// zero run), which is how the signed form of an L1 Transaction is hashed in place.
#pragma once
#include "bzk_field.cuh"
#include "bzk_gather.cuh"

namespace bzk {
namespace sha512 {

struct Msg {
    const uint8_t* p[3];
    uint64_t len[3];
    int32_t tail;  // < 0: none; else one more byte after the third range
};
struct Digest {
    uint32_t w[16];  // the 64 digest bytes as little-endian words: the limbs of the integer sc_reduce512 reduces
};

BZK_HD Msg msg_one(const uint8_t* p, uint64_t len) {
    Msg m;
    m.p[0] = p; m.len[0] = len;
    m.p[1] = p; m.len[1] = 0;
    m.p[2] = p; m.len[2] = 0;
    m.tail = -1;
    return m;
}

static constexpr uint64_t K[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
    0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
    0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
    0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
    0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
    0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
    0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

// rotation to the right by a constant 0 < N < 64, on the 32-bit halves
template <int N>
BZK_HD uint64_t rotr(uint64_t v) {
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    constexpr int S = N % 32;
    const uint32_t a = N < 32 ? lo : hi, b = N < 32 ? hi : lo;  // a rotation by 32 swaps the halves
    if constexpr (S == 0) return ((uint64_t)b << 32) | a;
    else return ((uint64_t)((b >> S) | (a << (32 - S))) << 32) | ((a >> S) | (b << (32 - S)));
}
BZK_HD uint64_t big_sigma0(uint64_t x) { return rotr<28>(x) ^ rotr<34>(x) ^ rotr<39>(x); }
BZK_HD uint64_t big_sigma1(uint64_t x) { return rotr<14>(x) ^ rotr<18>(x) ^ rotr<41>(x); }
BZK_HD uint64_t small_sigma0(uint64_t x) { return rotr<1>(x) ^ rotr<8>(x) ^ (x >> 7); }
BZK_HD uint64_t small_sigma1(uint64_t x) { return rotr<19>(x) ^ rotr<61>(x) ^ (x >> 6); }

// the byte at position pos of the padded message: message bytes, then 0x80, then zeros (the length words are set by the caller)
BZK_HD uint32_t byte_at(const Msg& m, uint64_t total, uint64_t pos) {
    if (pos >= total) return pos == total ? 0x80u : 0u;
    if (pos < m.len[0]) return m.p[0][pos];
    pos -= m.len[0];
    if (pos < m.len[1]) return m.p[1][pos];
    pos -= m.len[1];
    if (pos < m.len[2]) return m.p[2][pos];
    return (uint32_t)m.tail & 0xffu;
}
// the eight bytes at pos .. pos + 8 of the padded message as a big-endian word
BZK_HD uint64_t load_word(const Msg& m, uint64_t total, uint64_t pos) {
    const uint8_t* src = nullptr;
    const uint64_t e0 = m.len[0], e1 = e0 + m.len[1], e2 = e1 + m.len[2];
    if (pos + 8 <= e0) src = m.p[0] + pos;
    else if (pos >= e0 && pos + 8 <= e1) src = m.p[1] + (pos - e0);
    else if (pos >= e1 && pos + 8 <= e2) src = m.p[2] + (pos - e1);
    if (src) {
        uint64_t w;
        __builtin_memcpy(&w, src, 8);
        return __builtin_bswap64(w);
    }
    uint64_t w = 0;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) w = (w << 8) | byte_at(m, total, pos + k);  // rolled: the rare path stays small
    return w;
}

BZK_HD uint64_t msg_total(const Msg& m) { return m.len[0] + m.len[1] + m.len[2] + (m.tail >= 0 ? 1 : 0); }

// the same for a gathered message: its bytes read as zero past the end, so the 0x80 byte is set here
BZK_HD uint64_t msg_total(const gather::Msg& m) { return gather::total(m); }
BZK_HD uint64_t load_word(const gather::Msg& m, uint64_t total, uint64_t pos) {
    uint64_t w = gather::fetch8_be(m, pos);
    const uint64_t k = total - pos;  // wraps where pos > total
    if (k < 8) w |= (uint64_t)0x80 << (8 * (7 - k));
    return w;
}

#define BZK_SHA512_ROUND(a, b, c, d, e, f, g, h, i)                                                        \
    {                                                                                                      \
        if (t) w[i] += small_sigma1(w[(i + 14) & 15]) + w[(i + 9) & 15] + small_sigma0(w[(i + 1) & 15]);   \
        const uint64_t t1 = h + big_sigma1(e) + ((e & f) ^ (~e & g)) + K[16 * t + i] + w[i];               \
        const uint64_t t2 = big_sigma0(a) + ((a & b) ^ (a & c) ^ (b & c));                                 \
        d += t1;                                                                                           \
        h = t1 + t2;                                                                                       \
    }

template <class M>
BZK_HD Digest sha512_one(const M& m) {
    uint64_t s[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                     0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
    const uint64_t total = msg_total(m);
    const uint64_t blocks = (total + 144) / 128;  // the 0x80 byte and the 16 length bytes always fit the last block
#pragma unroll 1
    for (uint64_t blk = 0; blk < blocks; ++blk) {
        uint64_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = load_word(m, total, 128 * blk + 8 * i);
        if (blk + 1 == blocks) {  // the last sixteen bytes lie past the 0x80 byte: zeros so far
            w[14] = total >> 61;
            w[15] = total << 3;
        }
        uint64_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#pragma unroll 1
        for (int t = 0; t < 5; ++t) {
            BZK_SHA512_ROUND(a, b, c, d, e, f, g, h, 0)
            BZK_SHA512_ROUND(h, a, b, c, d, e, f, g, 1)
            BZK_SHA512_ROUND(g, h, a, b, c, d, e, f, 2)
            BZK_SHA512_ROUND(f, g, h, a, b, c, d, e, 3)
            BZK_SHA512_ROUND(e, f, g, h, a, b, c, d, 4)
            BZK_SHA512_ROUND(d, e, f, g, h, a, b, c, 5)
            BZK_SHA512_ROUND(c, d, e, f, g, h, a, b, 6)
            BZK_SHA512_ROUND(b, c, d, e, f, g, h, a, 7)
            BZK_SHA512_ROUND(a, b, c, d, e, f, g, h, 8)
            BZK_SHA512_ROUND(h, a, b, c, d, e, f, g, 9)
            BZK_SHA512_ROUND(g, h, a, b, c, d, e, f, 10)
            BZK_SHA512_ROUND(f, g, h, a, b, c, d, e, 11)
            BZK_SHA512_ROUND(e, f, g, h, a, b, c, d, 12)
            BZK_SHA512_ROUND(d, e, f, g, h, a, b, c, 13)
            BZK_SHA512_ROUND(c, d, e, f, g, h, a, b, 14)
            BZK_SHA512_ROUND(b, c, d, e, f, g, h, a, 15)
        }
        s[0] += a; s[1] += b; s[2] += c; s[3] += d; s[4] += e; s[5] += f; s[6] += g; s[7] += h;
    }
    Digest out;
#pragma unroll
    for (int i = 0; i < 8; ++i) {  // the digest is the state's words big-endian; out.w holds its bytes as little-endian words
        out.w[2 * i] = __builtin_bswap32((uint32_t)(s[i] >> 32));
        out.w[2 * i + 1] = __builtin_bswap32((uint32_t)s[i]);
    }
    return out;
}
#undef BZK_SHA512_ROUND

}  // namespace sha512
}  // namespace bzk
