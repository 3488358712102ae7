// Jubjub EdDSA key derivation and signing, one key or one signature per lane (sign.hip jubjub_keys_kernel / jubjub_sign_kernel; the CPU harness
// tests/host/eddsa_sign_check.hip runs the same code): the reference's `JubJub::generate_keys` and `JubJub::sign` (src/crypto/jubjub/mod.rs:112-150)
//     keys:  randomness = hash_to_scalar(seed),  scalar = hash_to_scalar(randomness.to_repr()),  pub = scalar BASE
//     sign:  r = Poseidon(randomness, msg),  R = r BASE,  h = Poseidon(R.x, R.y, pk.x, pk.y, msg),  s = (r + h a) mod ORDER
// Signing is deterministic, so the bytes equal the host signer's.  No lane shares anything with another and none uses LDS.
//
//   r BASE      unsigned radix-16 digits of the full integer r (below the field's modulus, NOT reduced modulo ORDER, as in the reference) against
//               the verifier's table j 16^i BASE (bzk_eddsa.cuh base_table_build): 64 mixed additions, no doublings, then one inversion for the
//               affine form.  The table is indexed by nibbles of the secret nonce (of the secret scalar for keys): the flow is fixed, the
//               addresses are not - a throughput signer, not a hardened one
//   mod ORDER   Barrett with respect to ORDER (252 bits): x = h a + r < 2^510, q = ((x >> 248) MU) >> 264 with MU = floor(2^512 / ORDER), which
//               is the quotient or up to two below it, so x - q ORDER < 3 ORDER < 2^254 is formed modulo 2^256 and two selects finish.  No
//               division and no data-dependent trip count
//
// Field products per signature (squares counted as products):
//   r = Poseidon, arity 2          8 full rounds x (9 + 9) + 56 partial x 8 + tail and conversions, about      610
//   r BASE                         64 x mixed add                      64 x 11                                  704
//   affine R                       inversion 254 squares + 164 products, 2 products, 2 conversions out          422
//   h = Poseidon, arity 5          as in bzk_eddsa.cuh, about                                                 1 260
//   s                              2 out of, 1 into Montgomery form (8 x 32-bit products), 181 word products      3      total about 3 000
// per key: two Keccak permutations per 136 seed bytes + one, 2 products into Montgomery form, 704 + 422 for pub     total about 1 130
#pragma once
#include "bzk_eddsa.cuh"
#include "bzk_keccak.cuh"

namespace bzk {
namespace eddsa {

// Jubjub's subgroup order and floor(2^512 / ORDER), little-endian 32-bit words
static constexpr uint32_t SC_ORDER[8] = {0xd6f72cb7u, 0xd0970e5eu, 0xccc81082u, 0xa6682093u, 0x01343b00u, 0x06673b01u, 0x6533afa9u, 0x0e7db4eau};
static constexpr uint32_t SC_MU[9] = {0xb2461ca9u, 0x77565ee9u, 0x2b99f029u, 0x1b7c7219u, 0x3f0476a0u, 0xc5aee5b8u, 0xf6f1bbe1u, 0xaa84a76fu, 0x00000011u};

// (r + h a) mod ORDER for canonical integers h, a, r below the field's modulus (limbs of plain integers, not Montgomery); the canonical
// representative, as Montgomery limbs (s travels as a ZkScalar)
BZK_HD Fr sc_muladd_mod_order(const Fr& h, const Fr& a, const Fr& r) {
    uint32_t x[17];  // h a + r < 2^510; x[16] = 0 pads the shift below
#pragma unroll
    for (int i = 0; i < 17; ++i) x[i] = i < 8 ? r.l[i] : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t t = (uint64_t)h.l[i] * a.l[j] + x[i + j] + carry;
            x[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
#pragma unroll
        for (int k = i + 8; k < 16; ++k) {  // r's words may already sit above the row: the carry runs on
            const uint64_t t = (uint64_t)x[k] + carry;
            x[k] = (uint32_t)t;
            carry = t >> 32;
        }
    }
    uint32_t q1[9], p[19];  // q1 = x >> 248 < 2^262; p = q1 MU < 2^523; p[18] = 0 pads the shift below
#pragma unroll
    for (int i = 0; i < 9; ++i) q1[i] = (x[7 + i] >> 24) | (x[8 + i] << 8);
#pragma unroll
    for (int i = 0; i < 19; ++i) p[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const uint64_t t = (uint64_t)q1[i] * SC_MU[j] + p[i + j] + carry;
            p[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
        p[i + 9] = (uint32_t)carry;
    }
    uint32_t q[8], m[8];  // the low 256 bits of q = p >> 264 and of q ORDER: the difference below is less than 2^254
#pragma unroll
    for (int i = 0; i < 8; ++i) q[i] = (p[8 + i] >> 8) | (p[9 + i] << 24);
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j + i < 8; ++j) {
            const uint64_t t = (uint64_t)q[i] * SC_ORDER[j] + m[i + j] + carry;
            m[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
    }
    Fr out;
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)x[i] - m[i] - borrow;
        out.l[i] = (uint32_t)d;
        borrow = (d >> 63) & 1;
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t d[8];
        borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t y = (uint64_t)out.l[i] - SC_ORDER[i] - borrow;
            d[i] = (uint32_t)y;
            borrow = (y >> 63) & 1;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) out.l[i] = borrow ? out.l[i] : d[i];
    }
    return fe_to_mont<FrParams>(out);
}

// k BASE as affine Montgomery-256 limbs for a canonical integer k below the field's modulus (64 nibbles): 64 mixed additions over base_tab
// (bzk_eddsa.cuh base_table_build), one inversion (Z is never zero: the addition law is complete)
BZK_HD void base_mul_affine(Fr k, const Fr29* __restrict__ base_tab, Fr* __restrict__ xy) {
    const Fr29 dc = base_tab[BASE_TAB_LEN - 1], one = fr29::from_consts(fr29::ONE);
    wf::JP acc = {fr29::zero(), one, one};
#pragma unroll 1
    for (int w = 0; w < FWIN; ++w) {
        const Fr29* e = base_tab + ((size_t)w * FTAB + (k.l[0] & (FTAB - 1u))) * 2;
#pragma unroll
        for (int i = 0; i < 7; ++i) k.l[i] = (k.l[i] >> FW) | (k.l[i + 1] << (32 - FW));
        k.l[7] >>= FW;
        acc = wf::jp_add_affine(acc, e[0], e[1], dc);
    }
    const Fr29 zi = fr29::inv(acc.Z);
    xy[0] = fr29::from29(fr29::mul(acc.X, zi));
    xy[1] = fr29::from29(fr29::mul(acc.Y, zi));
}

// One signature.  key = pub.x | pub.y | randomness | scalar, msg, sig = r.x | r.y | s (Montgomery-256 limbs); c3 / c6: the sparse Poseidon
// constants of widths 3 and 6 (bzk_poseidon29.cuh).  pub is taken as given.  A field of key or msg that is not the limbs of a residue gives 0
// and a zero signature (the lane then runs on zeros, as verify_one does, so that the field's bounds hold for any input).
BZK_HD uint8_t sign_one(const Fr* __restrict__ key, const Fr* __restrict__ msg, const Fr29* __restrict__ c3, int rf3, int rp3,
                        const Fr29* __restrict__ c6, int rf6, int rp6, const Fr29* __restrict__ base_tab, Fr* __restrict__ sig) {
    bool ok = canonical(msg[0]);
#pragma unroll
    for (int i = 0; i < 4; ++i) ok = ok && canonical(key[i]);
    const Fr z = Fr::zero();
    const Fr m = fr_sel(ok, msg[0], z);
    Fr rc;  // the nonce as an integer
    {
        const Fr in[2] = {fr_sel(ok, key[2], z), m};
        rc = fe_from_mont<FrParams>(poseidon29_hash<3>(in, c3, rf3, rp3));
    }
    Fr in[5];
    base_mul_affine(rc, base_tab, in);
    // pk and the scalar are read again here, through a pointer the compiler cannot see through, instead of being carried across the walk above
    BZK_EDDSA_OPAQUE(key);
    in[2] = fr_sel(ok, key[0], z);
    in[3] = fr_sel(ok, key[1], z);
    in[4] = m;
    const Fr hc = fe_from_mont<FrParams>(poseidon29_hash<6>(in, c6, rf6, rp6));
    const Fr s = sc_muladd_mod_order(hc, fe_from_mont<FrParams>(fr_sel(ok, key[3], z)), rc);
    sig[0] = fr_sel(ok, in[0], z);
    sig[1] = fr_sel(ok, in[1], z);
    sig[2] = fr_sel(ok, s, z);
    return ok ? 1 : 0;
}

// SHA3-256 of 32 bytes given as eight little-endian words: less than one block, so one permutation
BZK_HD keccak::Digest sha3_256_words8(const uint32_t* a) {
    keccak::State st;
#pragma unroll
    for (int i = 0; i < 4; ++i) st.s[i] = (uint64_t)a[2 * i] | ((uint64_t)a[2 * i + 1] << 32);
    st.s[4] = 0x06;
#pragma unroll
    for (int i = 5; i < 25; ++i) st.s[i] = 0;
    st.s[16] = (uint64_t)0x80 << 56;
    keccak::permute(st);
    return keccak::squeeze(st);
}

// One key from seed[0 .. len): key = pub.x | pub.y | randomness | scalar (the layout of bzk_host_jubjub_keys)
BZK_HD void keys_one(const uint8_t* __restrict__ seed, uint64_t len, const Fr29* __restrict__ base_tab, Fr* __restrict__ key) {
    const Fr randomness = keccak::fr_from_le_bytes_mod(keccak::sha3_256_one(seed, len, keccak::NO_BLANK));
    const Fr repr = fe_from_mont<FrParams>(randomness);  // to_repr(): the canonical integer's little-endian bytes
    const Fr scalar = keccak::fr_from_le_bytes_mod(sha3_256_words8(repr.l));
    base_mul_affine(fe_from_mont<FrParams>(scalar), base_tab, key);
    key[2] = randomness;
    key[3] = scalar;
}

// Whether the compressed key (x, odd) of a record is the compression of the affine point pub (both as Montgomery-256 limbs; pub's fields
// residues' limbs): the same x, and odd = the parity of the canonical integer of pub.y (`PointAffine::compress`, src/crypto/jubjub/curve.rs:70-76)
BZK_HD bool compresses_to(const Fr* __restrict__ pub, const Fr& x, bool odd) {
    const bool is_odd = (fe_from_mont<FrParams>(pub[1]).l[0] & 1u) != 0;
    return pub[0].equals(x) && is_odd == odd;
}

}  // namespace eddsa
}  // namespace bzk
