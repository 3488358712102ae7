// SHA3-256 and `hash_to_scalar` (src/zk/mod.rs:218-220), one message per lane (eddsa.hip sha3_256_kernel; the CPU harness
// tests/host/keccak_check.hip runs the same code).  FIPS 202: Keccak-f[1600], rate 136 bytes, domain suffix 0x06, final bit 0x80.
//
// The 25 lanes of the state are 64-bit values that every access names with a constant index (the loops over them are fully unrolled and the
// rotation amounts / the pi permutation are compile-time tables), so they live in 50 registers; only the loop over the 24 rounds is kept rolled
// (its round constant is a uniform load), which keeps the kernel's text at one round plus the absorb code.  A lane loops over as many 136-byte
// blocks as its own message has: lanes of one wave with different lengths diverge at the block loop's exit only.
//
// Bytes are fetched eight at a time where the word lies wholly inside the message and outside the blanked range, byte by byte otherwise (the
// message's tail and the words the blanked range touches).  The blanked range is how ContractWithdraw::fingerprint (src/core/transaction.rs:204-211)
// hashes the payment "with calldata := 0" without a copy of the payment.
//
// The absorb loop is a template on where its words come from: the flat message with its blanked range, or a gathered message (bzk_gather.cuh),
// which is how Transaction::hash (src/core/transaction.rs:383-385) hashes a record's signed form in place.  sha3_256_pair is the 64-byte case
// of the block's Merkle tree (src/crypto/merkle.rs:9-19): one permutation.
#pragma once
#include <utility>

#include "bzk_field.cuh"
#include "bzk_gather.cuh"

namespace bzk {
namespace keccak {

constexpr int RATE = 136;                      // bytes per absorbed block: 17 lanes
constexpr uint64_t NO_BLANK = ~(uint64_t)0;    // blank_off: nothing is blanked
constexpr uint64_t BLANK_LEN = 32;             // the blanked range's length (a ZkScalar)

struct State {
    uint64_t s[25];  // lane (x, y) at s[x + 5 y]
};
struct Digest {
    uint32_t w[8];  // the 32 digest bytes as little-endian words: also the limbs of the integer `ZkScalar::new` reduces
};

static constexpr uint64_t RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

// rho: rotation of lane x + 5 y
struct Rho {
    int v[25];
};
static constexpr Rho RHO = {{0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14}};

// rotation by a constant, on the 32-bit halves: each half of the result is one funnel shift of the two input halves (v_alignbit_b32), where
// the 64-bit form compiles to a 64-bit shift, a 32-bit shift and an or
template <int N>
BZK_HD uint64_t rotl(uint64_t v) {
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    constexpr int K = N % 32;
    const uint32_t a = N < 32 ? lo : hi, b = N < 32 ? hi : lo;  // a rotation by 32 swaps the halves
    if constexpr (K == 0) return ((uint64_t)b << 32) | a;
    else return ((uint64_t)((b << K) | (a >> (32 - K))) << 32) | ((a << K) | (b >> (32 - K)));
}

// pi after rho: B[y + 5 ((2 x + 3 y) mod 5)] = rotl(A[x + 5 y], RHO[x + 5 y])
template <int I>
BZK_HD void rho_pi_lane(const State& a, State& b) {
    constexpr int x = I % 5, y = I / 5;
    b.s[y + 5 * ((2 * x + 3 * y) % 5)] = rotl<RHO.v[I]>(a.s[I]);
}
template <int... I>
BZK_HD void rho_pi_all(const State& a, State& b, std::integer_sequence<int, I...>) {
    (rho_pi_lane<I>(a, b), ...);
}

BZK_HD void round_one(State& a, uint64_t rc) {
    uint64_t c[5], d[5];
#pragma unroll
    for (int x = 0; x < 5; ++x) c[x] = a.s[x] ^ a.s[x + 5] ^ a.s[x + 10] ^ a.s[x + 15] ^ a.s[x + 20];
#pragma unroll
    for (int x = 0; x < 5; ++x) d[x] = c[(x + 4) % 5] ^ rotl<1>(c[(x + 1) % 5]);
#pragma unroll
    for (int i = 0; i < 25; ++i) a.s[i] ^= d[i % 5];
    State b;
    rho_pi_all(a, b, std::make_integer_sequence<int, 25>());
#pragma unroll
    for (int y = 0; y < 5; ++y) {
#pragma unroll
        for (int x = 0; x < 5; ++x) a.s[x + 5 * y] = b.s[x + 5 * y] ^ (~b.s[(x + 1) % 5 + 5 * y] & b.s[(x + 2) % 5 + 5 * y]);
    }
    a.s[0] ^= rc;
}

BZK_HD void permute(State& a) {
#pragma unroll 1
    for (int r = 0; r < 24; ++r) round_one(a, RC[r]);
}

// the eight message bytes at pos .. pos + 8 as a little-endian word: bytes at or past len read as 0, bytes inside the blanked range read as 0
BZK_HD uint64_t load_word(const uint8_t* __restrict__ data, uint64_t len, uint64_t pos, uint64_t blank_off) {
    const bool inside = pos + 8 <= len;
    const bool touches = blank_off != NO_BLANK && pos + 8 > blank_off && pos < blank_off + BLANK_LEN;
    uint64_t w = 0;
    if (inside && !touches) {
        __builtin_memcpy(&w, data + pos, 8);
        return w;
    }
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {  // rolled: the rare path (a message's last word, the words the blanked range touches) stays small
        const uint64_t p = pos + k;
        const bool blanked = blank_off != NO_BLANK && p >= blank_off && p < blank_off + BLANK_LEN;
        if (p < len && !blanked) w |= (uint64_t)data[p] << (8 * k);
    }
    return w;
}

// where the absorb loop's words come from: load(pos) = the eight message bytes at pos as a little-endian word, zeros at or past the end
struct FlatWords {
    const uint8_t* __restrict__ data;
    uint64_t len, blank_off;
    BZK_HD uint64_t operator()(uint64_t pos) const { return load_word(data, len, pos, blank_off); }
};
struct GatheredWords {
    const gather::Msg& m;
    BZK_HD uint64_t operator()(uint64_t pos) const { return gather::fetch8_le(m, pos); }
};

BZK_HD Digest squeeze(const State& a) {
    Digest d;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        d.w[2 * i] = (uint32_t)a.s[i];
        d.w[2 * i + 1] = (uint32_t)(a.s[i] >> 32);
    }
    return d;
}

template <class Words>
BZK_HD Digest sha3_256_absorb(uint64_t len, const Words& load) {
    State a;
#pragma unroll
    for (int i = 0; i < 25; ++i) a.s[i] = 0;
    const uint64_t blocks = len / RATE + 1;  // the padding always adds its bits: a message of a whole number of blocks gets one more
#pragma unroll 1
    for (uint64_t b = 0; b < blocks; ++b) {
        const uint64_t base = b * RATE;
        const bool last = b + 1 == blocks;
        const uint64_t rem = len - base;  // only meaningful in the last block: 0 .. 135 message bytes in it
#pragma unroll
        for (int w = 0; w < 17; ++w) {
            uint64_t v = load(base + 8 * w);
            if (last) {
                if ((rem >> 3) == (uint64_t)w) v ^= (uint64_t)0x06 << (8 * (rem & 7));
                if (w == 16) v ^= (uint64_t)0x80 << 56;
            }
            a.s[w] ^= v;
        }
        permute(a);
    }
    return squeeze(a);
}

// SHA3-256 of data[0 .. len) with the 32 bytes at blank_off (NO_BLANK: none) absorbed as zeros
BZK_HD Digest sha3_256_one(const uint8_t* __restrict__ data, uint64_t len, uint64_t blank_off) {
    return sha3_256_absorb(len, FlatWords{data, len, blank_off});
}
// SHA3-256 of a gathered message
BZK_HD Digest sha3_256_one(const gather::Msg& m) { return sha3_256_absorb(gather::total(m), GatheredWords{m}); }

// SHA3-256 of the 64 bytes a | b (each eight little-endian words): less than one block, so one permutation
BZK_HD Digest sha3_256_pair(const uint32_t* a, const uint32_t* b) {
    State st;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        st.s[i] = (uint64_t)a[2 * i] | ((uint64_t)a[2 * i + 1] << 32);
        st.s[4 + i] = (uint64_t)b[2 * i] | ((uint64_t)b[2 * i + 1] << 32);
    }
    st.s[8] = 0x06;
#pragma unroll
    for (int i = 9; i < 25; ++i) st.s[i] = 0;
    st.s[16] = (uint64_t)0x80 << 56;
    permute(st);
    return squeeze(st);
}

// ZkScalar::new (src/zk/mod.rs:263-270) of a 32-byte little-endian integer: its residue in Montgomery form.  2^256 < 3 r, so two conditional
// subtractions of r (selects) bring it below r; one product by R^2 then makes the Montgomery form.
BZK_HD Fe<FrParams> fr_from_le_bytes_mod(const Digest& d) {
    Fe<FrParams> v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v.l[i] = d.w[i];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t t[8];
        uint64_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t x = (uint64_t)v.l[i] - FrParams::MOD[i] - borrow;
            t[i] = (uint32_t)x;
            borrow = (x >> 63) & 1;
        }
        const uint32_t keep = (uint32_t)0 - (uint32_t)borrow;  // all ones where v < r: v stays
#pragma unroll
        for (int i = 0; i < 8; ++i) v.l[i] = (v.l[i] & keep) | (t[i] & ~keep);
    }
    return fe_to_mont<FrParams>(v);
}

}  // namespace keccak
}  // namespace bzk
