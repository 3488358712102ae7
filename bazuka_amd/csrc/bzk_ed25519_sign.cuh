// Ed25519 key derivation and signing as the reference does them (src/crypto/ed25519.rs:70-80 over `ed25519-dalek = "1"`: `Keypair::sign` is
// RFC 8032 5.1.6), one row per lane (ed_sign.hip's kernels; the CPU harness tests/host/ed25519_sign_check.hip and the ctx = NULL entries run the
// same code).  Field, group, table and reduction are the verifier's (bzk_ed25519.cuh); this file adds the expansion of a secret, the fixed-base
// product with its encoding, the multiply-add modulo l and the two rows built from them.
//
//   expand:  h = SHA-512(secret); a = h[0 .. 32) clamped; prefix = h[32 .. 64)
//   sign:    r = SHA-512(prefix | M) mod l; R = encode([r]B); k = SHA-512(R | A | M) mod l; s = (k a + r) mod l; the signature is R | s
//   keys:    secret = SHA3-256(seed) with bit 255 cleared; public = encode([a]B); the key is secret | public (`Keypair::to_bytes`)
//
// SHA-512 reads its message through pointers, and prefix and R are a lane's own values: they go through memory the lane owns (a row of the
// call's workspace, the row of the output) and are read back from there by the lane that stored them, so nothing per lane is indexed in
// registers and no kernel needs a private segment.
#pragma once
#include "bzk_ed25519.cuh"
#include "bzk_keccak.cuh"

namespace bzk {
namespace ed25519 {

constexpr int EXPANDED_BYTES = 64;  // a | prefix, a row of the workspace

BZK_HD void store_words8(uint8_t* p, const uint32_t (&w)[8]) {  // any alignment
#pragma unroll
    for (int i = 0; i < 8; ++i) __builtin_memcpy(p + 4 * i, &w[i], 4);
}
// the low half of SHA-512(secret) as the secret scalar: a multiple of 8 in [2^254, 2^255)
BZK_HD void clamp(uint32_t (&a)[8]) {
    a[0] &= ~7u;
    a[7] = (a[7] & 0x7fffffffu) | 0x40000000u;
}
// a | prefix of the 32-byte secret at `secret`
BZK_HD void expand(const uint8_t* secret, uint32_t (&a)[8], uint32_t (&prefix)[8]) {
    const sha512::Digest h = sha512::sha512_one(sha512::msg_one(secret, 32));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = h.w[i];
        prefix[i] = h.w[8 + i];
    }
    clamp(a);
}
BZK_HD void expand_store(const uint8_t* secret, uint8_t* exp) {
    uint32_t a[8], prefix[8];
    expand(secret, a, prefix);
    store_words8(exp, a);
    store_words8(exp + 32, prefix);
}

// encode([k]B) for the 256-bit integer k, not reduced: the verifier's walk over all 64 nibbles (the table holds j 16^i B up to i = 63), 64 mixed
// additions, no doubling, the one inversion inside encode.  The nibble is always the lowest of k, which moves down four bits per step: every
// index into k is a constant.
BZK_HD void base_mul_encode(const uint32_t (&scalar)[8], const uint32_t* __restrict__ base_tab, uint32_t (&out)[8]) {
    uint32_t k[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = scalar[i];
    Pt q = pt_identity();
#pragma unroll 1
    for (int i = 0; i < BASE_WINDOWS; ++i) {
        const uint32_t* e = base_tab + ((size_t)i * BASE_ENTRIES + (k[0] & 15u)) * NIELS_WORDS;
#pragma unroll
        for (int j = 0; j < 7; ++j) k[j] = (k[j] >> 4) | (k[j + 1] << 28);
        k[7] >>= 4;
        q = pt_add_niels(q, fe_load(e, 1), fe_load(e + 10, 1), fe_load(e + 20, 1));
    }
    encode(q, out);
}

// (k a + r) mod l for any three 256-bit integers: k a + r <= (2^256 - 1)^2 + 2^256 - 1 < 2^512 (signing has k, r < l and a < 2^255: below 2^508).
// The sixteen words go through the verifier's sc_reduce512, whose bounds hold for EVERY 512-bit input x, not only for digests:
//   hi = x >> 252 < 2^260 (nine words); t = hi c < 2^260 2^125 = 2^385 (thirteen words); thi = t >> 252 < 2^133 (six words);
//   u = thi c < 2^258 (ten words); uhi = u >> 252 < 2^6; v = uhi c < 2^131 (seven words);
//   x = lo - tlo + ulo - v (mod l) with lo, tlo, ulo < 2^252, so lo + ulo + 2 l - tlo - v lies in (2 l - 2^252 - 2^131, 2^253 + 2 l), which is
//   inside (0, 4 l) because 2^252 < l: no borrow, no carry out of eight words (4 l < 2^255), and three of its four conditional subtractions
//   of l bring it below l.
// Fixed flow: an 8 x 8-word schoolbook product, no division, no data-dependent trip count.
BZK_HD void sc_muladd(const uint32_t (&k)[8], const uint32_t (&a)[8], const uint32_t (&r)[8], uint32_t (&out)[8]) {
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = i < 8 ? r[i] : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t v = (uint64_t)k[i] * a[j] + x[i + j] + carry;  // at most (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
            x[i + j] = (uint32_t)v;
            carry = v >> 32;
        }
        x[i + 8] = (uint32_t)carry;  // still zero before this row: r fills the low eight words only
    }
    sc_reduce512(x, out);
}

// SHA-512(prefix | M), the nonce's hash.  A sha512::Msg body (one range and an optional literal byte, as hash_ram takes it) gets the 32 bytes at
// `prefix` in front; a gathered body carries them as its first piece already (signed_form_prefixed below).
BZK_HD sha512::Digest hash_prefixed(const uint8_t* prefix, const sha512::Msg& body) {
    sha512::Msg m;
    m.p[0] = prefix; m.len[0] = 32;
    m.p[1] = body.p[0]; m.len[1] = body.len[0];
    m.p[2] = body.p[0]; m.len[2] = 0;
    m.tail = body.tail;
    return sha512::sha512_one(m);
}
BZK_HD sha512::Digest hash_prefixed(const uint8_t*, const gather::Msg& body) { return sha512::sha512_one(body); }

// gather::signed_form with one 32-byte piece (at front_off from base) in front instead of R | A: what the nonce of an L1 transaction hashes
BZK_HD gather::Msg signed_form_prefixed(const uint8_t* base, uint32_t rec_off, uint32_t cut_a, uint32_t cut_b, uint32_t sig_tag, uint32_t front_off) {
    const bool cut = cut_a != cut_b;
    gather::Msg m = gather::msg_empty(base);
    gather::set_piece<0>(m, front_off, 32);
    gather::set_piece<1>(m, rec_off, cut ? cut_a : sig_tag);
    gather::set_piece<2>(m, gather::ZEROS, cut ? 1 : 0);
    gather::set_piece<3>(m, rec_off + cut_b, cut ? sig_tag - cut_b : 0);
    gather::set_piece<4>(m, gather::ZEROS, 4);
    gather::set_piece<5>(m, gather::ZEROS, 0);
    return m;
}

// One signature.  exp: the key's a | prefix (expand_store's 64 bytes); pk: A's 32 bytes, taken as given (dalek's ExpandedSecretKey::sign does the
// same); sig: 64 bytes the lane owns.  body_r is what follows the prefix in the first hash and body_k what follows R | A in the second: for a
// sha512::Msg both are the message itself; gathered bodies carry prefix and R | A as their first pieces, R's being the 32 bytes at sig.
// R is stored to sig before the second hash reads it from there: the same lane, the same address, program order.
template <class Body>
BZK_HD void sign_one(const uint8_t* exp, const uint8_t* pk, const Body& body_r, const Body& body_k, const uint32_t* __restrict__ base_tab,
                     uint8_t* sig) {
    uint32_t r[8];
    {
        const sha512::Digest h = hash_prefixed(exp + 32, body_r);
        sc_reduce512(h.w, r);
    }
    {
        uint32_t enc[8];
        base_mul_encode(r, base_tab, enc);
        store_words8(sig, enc);
    }
    uint32_t k[8], a[8], s[8];
    {
        const sha512::Digest h = hash_ram(pk, sig, body_k);
        sc_reduce512(h.w, k);
    }
    load_words8(exp, a);
    sc_muladd(k, a, r, s);
    store_words8(sig + 32, s);
}

// One key from seed[0 .. len): key = secret | public, 64 bytes the lane owns.  The secret is stored first and expanded from there.
BZK_HD void keys_one(const uint8_t* __restrict__ seed, uint64_t len, const uint32_t* __restrict__ base_tab, uint8_t* key) {
    {
        keccak::Digest d = keccak::sha3_256_one(seed, len, keccak::NO_BLANK);
        d.w[7] &= 0x7fffffffu;  // secret[31] &= 0x7f
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = d.w[i];
        store_words8(key, w);
    }
    uint32_t a[8], prefix[8], pub[8];
    expand(key, a, prefix);
    (void)prefix;
    base_mul_encode(a, base_tab, pub);
    store_words8(key + 32, pub);
}

// whether the 32 bytes at x and at y are equal (any alignment)
BZK_HD bool bytes32_equal(const uint8_t* x, const uint8_t* y) {
    uint32_t a[8], b[8], diff = 0;
    load_words8(x, a);
    load_words8(y, b);
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= a[i] ^ b[i];
    return diff == 0;
}

}  // namespace ed25519
}  // namespace bzk
