// Batched Jubjub EdDSA verification on the device (bzk_jubjub_verify_batch[_dev]): `JubJub::<ZkHasher>::verify` (src/crypto/jubjub/mod.rs:151-167) for
// n independent (key, message, signature) triples, one lane per signature.  The arithmetic is bzk_eddsa.cuh's verify_one; this file holds the kernel,
// the per-context table of multiples of BASE and the two entry points.

// The hash is a quarter of a verification and shares its kernel with the ladders: its MDS matrix is re-read in every full round (scalar loads) instead of
// being hoisted out of the round loop into 324 scalars the register file does not have (bzk_poseidon29.cuh)
#define BZK_POSEIDON_MDS_RELOAD 1
#include "bzk_decompress.cuh"
#include "bzk_keccak.cuh"
#include "bzk_ed25519.cuh"
#include "bzk_l1.cuh"
#include "bzk_internal.h"
#include "bzk_stage.h"
#include "host_threads.h"

namespace bzk {

int32_t poseidon_consts_dev_shared(bzk_ctx* ctx, int t, const void** out, int* rf, int* rp);  // poseidon.hip
int32_t poseidon_launch(bzk_ctx* ctx, const void* in_dev, uint32_t arity, uint64_t n, void* out_dev);       // poseidon.hip

// One wave per block: the lanes share nothing but the block's LDS, where lane l keeps its table {1, 2, 3, 4} pk in column l (word k at lds[64 k + l]:
// consecutive lanes, consecutive banks).  27 KB per block, five blocks per CU.
constexpr int EDDSA_BLOCK = 64;
__global__ void __launch_bounds__(EDDSA_BLOCK) jubjub_verify_kernel(const Fr* __restrict__ pub, const Fr* __restrict__ msg, const Fr* __restrict__ sig,
                                                                    uint64_t n, const Fr29* __restrict__ pconsts, int rf, int rp,
                                                                    const Fr29* __restrict__ base_tab, uint8_t* __restrict__ ok) {
    __shared__ uint32_t lds[eddsa::TAB_WORDS * EDDSA_BLOCK];
    const uint64_t i = (uint64_t)blockIdx.x * EDDSA_BLOCK + threadIdx.x;
    if (i >= n) return;
    ok[i] = eddsa::verify_one(pub + 2 * i, msg + i, sig + 3 * i, pconsts, rf, rp, base_tab, lds + threadIdx.x, EDDSA_BLOCK);
}

// Key decompression, one lane per key (bzk_decompress.cuh decompress_one): a dependent chain of about a thousand products in some sixty registers
// and no LDS, so blocks of four waves and as many waves per SIMD as the register count allows hide the chain's latency.
constexpr int DECOMPRESS_BLOCK = 256;
__global__ void __launch_bounds__(DECOMPRESS_BLOCK) jubjub_decompress_kernel(const Fr* __restrict__ x, const uint8_t* __restrict__ odd, uint64_t n,
                                                                             Fr* __restrict__ xy, uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * DECOMPRESS_BLOCK + threadIdx.x;
    if (i >= n) return;
    Fr o[2];
    ok[i] = eddsa::decompress_one(x[i], odd[i] != 0, o);
    xy[2 * i] = o[0];
    xy[2 * i + 1] = o[1];
}

// The hash inputs of m parsed transactions (tuples: m x 7 scalars) from their integers, token ids and the decompressed dst keys; fit[i] = whether
// record i can verify at all (tx_tuple_one)
__global__ void __launch_bounds__(256) mpn_tx_tuple_kernel(const uint64_t* __restrict__ nums, const Fr* __restrict__ tok, const Fr* __restrict__ dst_xy,
                                                           const uint8_t* __restrict__ dst_ok, uint64_t m, Fr* __restrict__ tuples,
                                                           uint8_t* __restrict__ fit) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    Fr t[7];
    fit[i] = eddsa::tx_tuple_one(nums + 3 * i, tok + 2 * i, dst_xy + 2 * i, dst_ok[i], t) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) tuples[7 * i + k] = t[k];
}
// ok[i] = verified and src decompressed and the record fit; the hash of a record that did not fit is zeros
__global__ void __launch_bounds__(256) mpn_tx_verdict_kernel(const uint8_t* __restrict__ verified, const uint8_t* __restrict__ src_ok,
                                                             const uint8_t* __restrict__ fit, uint64_t m, Fr* __restrict__ hash, uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    ok[i] = (verified[i] && src_ok[i] && fit[i]) ? 1 : 0;
    if (!fit[i]) hash[i] = Fr::zero();
}

// SHA3-256, one lane per message (bzk_keccak.cuh sha3_256_one): message i = data[begin[i] - base .. end[i] - base); blank (may be null): the
// offset inside message i of 32 bytes absorbed as zeros.  The state is 50 registers and the rounds are integer work with no memory traffic, so
// blocks of four waves; a lane's loads are its own message's bytes (neighbouring lanes are a message apart: nothing coalesces, and at about ten
// thousand instructions per 136 bytes nothing needs to).  digest (n x 8 words) and scalar (n, hash_to_scalar) may each be null.
constexpr int SHA3_BLOCK = 256;
__global__ void __launch_bounds__(SHA3_BLOCK) sha3_256_kernel(const uint8_t* __restrict__ data, const uint64_t* __restrict__ begin,
                                                              const uint64_t* __restrict__ end, uint64_t base, const uint32_t* __restrict__ blank,
                                                              uint64_t n, uint32_t* __restrict__ digest, Fr* __restrict__ scalar) {
    const uint64_t i = (uint64_t)blockIdx.x * SHA3_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = begin[i], e = end[i];
    const uint64_t len = e > b ? e - b : 0;
    const keccak::Digest d = keccak::sha3_256_one(data + (b - base), len, blank ? (uint64_t)blank[i] : keccak::NO_BLANK);
    if (digest) {
#pragma unroll
        for (int k = 0; k < 8; ++k) digest[8 * i + k] = d.w[k];
    }
    if (scalar) scalar[i] = keccak::fr_from_le_bytes_mod(d);
}

// The two hash inputs of m parsed MpnWithdraws: h2 = (fingerprint, nonce) for the signed message (transaction.rs:183-189), h6 = (address.x,
// address.y, nonce, r.x, r.y, s) for the calldata (:177-182); the nonce is brought into Montgomery form here.  fit[i] = whether record i can
// verify at all: the key decompressed and the signature's scalars are residues' limbs; zeros are hashed otherwise.
__global__ void __launch_bounds__(256) mpn_withdraw_inputs_kernel(const Fr* __restrict__ fp, const uint32_t* __restrict__ nonce,
                                                                  const Fr* __restrict__ xy, const uint8_t* __restrict__ key_ok,
                                                                  const Fr* __restrict__ sig, uint64_t m, Fr* __restrict__ h2, Fr* __restrict__ h6,
                                                                  uint8_t* __restrict__ fit) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const Fr r_x = sig[3 * i], r_y = sig[3 * i + 1], s = sig[3 * i + 2];
    const bool ok = key_ok[i] != 0 && eddsa::canonical(r_x) && eddsa::canonical(r_y) && eddsa::canonical(s);
    Fr c = Fr::zero();
    c.l[0] = nonce[i];
    const Fr nm = fe_to_mont<FrParams>(c), z = Fr::zero();
    h2[2 * i] = fp[i];
    h2[2 * i + 1] = nm;
    h6[6 * i] = eddsa::fr_sel(ok, xy[2 * i], z);
    h6[6 * i + 1] = eddsa::fr_sel(ok, xy[2 * i + 1], z);
    h6[6 * i + 2] = eddsa::fr_sel(ok, nm, z);
    h6[6 * i + 3] = eddsa::fr_sel(ok, r_x, z);
    h6[6 * i + 4] = eddsa::fr_sel(ok, r_y, z);
    h6[6 * i + 5] = eddsa::fr_sel(ok, s, z);
    fit[i] = ok ? 1 : 0;
}
// ok[i]: bit 0 = the signature verified, bit 1 = the payment's 32 calldata bytes (at data[begin[i] + cd[i]], any alignment) equal the limbs of
// H6's output as bytes; 0 where the record did not fit
__global__ void __launch_bounds__(256) mpn_withdraw_verdict_kernel(const uint8_t* __restrict__ verified, const uint8_t* __restrict__ fit,
                                                                   const Fr* __restrict__ h6, const uint8_t* __restrict__ data,
                                                                   const uint64_t* __restrict__ begin, const uint32_t* __restrict__ cd, uint64_t m,
                                                                   uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const uint8_t* p = data + begin[i] + cd[i];
    const Fr h = h6[i];
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t w = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
        diff |= w ^ h.l[k];
    }
    ok[i] = fit[i] ? (uint8_t)((verified[i] ? 1 : 0) | (diff == 0 ? 2 : 0)) : 0;
}

// SHA-512, one lane per message (bzk_sha512.cuh sha512_one): message i = data[begin[i] - base .. end[i] - base).  State and schedule ring are 48
// registers and the rounds are integer work, so blocks of four waves as for SHA3; lanes of a wave leave the block loop at their own trip.
constexpr int SHA512_BLOCK = 256;
__global__ void __launch_bounds__(SHA512_BLOCK) sha512_kernel(const uint8_t* __restrict__ data, const uint64_t* __restrict__ begin,
                                                              const uint64_t* __restrict__ end, uint64_t base, uint64_t n,
                                                              uint32_t* __restrict__ digest) {
    const uint64_t i = (uint64_t)blockIdx.x * SHA512_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = begin[i], e = end[i];
    const sha512::Digest d = sha512::sha512_one(sha512::msg_one(data + (b - base), e > b ? e - b : 0));
#pragma unroll
    for (int k = 0; k < 16; ++k) digest[16 * i + k] = d.w[k];
}

// Ed25519, one lane per signature (bzk_ed25519.cuh verify_one): hash, reduction and group equation in one kernel.  Key i is the 32 bytes at
// pk[pk_at[i]] (pk_at null: 32 i), signature i the 64 bytes at sig[sig_at[i]] (null: 64 i), message i = data[begin[i] - base .. end[i] - base)
// followed by the byte `tail` where tail >= 0.  One wave per block: lane l keeps its table and its two scalars in column l of the block's LDS
// (word k at lds[64 k + l]), 45 312 bytes per block, three blocks per CU.
constexpr int ED25519_BLOCK = 64;
__global__ void __launch_bounds__(ED25519_BLOCK) ed25519_verify_kernel(const uint8_t* __restrict__ pk, const uint64_t* __restrict__ pk_at,
                                                                       const uint8_t* __restrict__ sig, const uint64_t* __restrict__ sig_at,
                                                                       const uint8_t* __restrict__ data, const uint64_t* __restrict__ begin,
                                                                       const uint64_t* __restrict__ end, uint64_t base, int32_t tail, uint64_t n,
                                                                       const uint32_t* __restrict__ base_tab, uint8_t* __restrict__ ok) {
    __shared__ uint32_t lds[ed25519::LANE_WORDS * ED25519_BLOCK];
    const uint64_t i = (uint64_t)blockIdx.x * ED25519_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = begin[i], e = end[i];
    sha512::Msg body = sha512::msg_one(data + (b - base), e > b ? e - b : 0);
    body.tail = tail;
    ok[i] = ed25519::verify_one(pk + (pk_at ? pk_at[i] : 32 * i), sig + (sig_at ? sig_at[i] : 64 * i), body, base_tab, lds + threadIdx.x,
                                ED25519_BLOCK);
}
// ok[i]: bit 0 = the payment carries a signature and it verified, bit 1 = mpn_address decompressed
__global__ void __launch_bounds__(256) mpn_deposit_verdict_kernel(const uint8_t* __restrict__ verified, const uint8_t* __restrict__ has_sig,
                                                                  const uint8_t* __restrict__ key_ok, uint64_t m, uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    ok[i] = (uint8_t)((verified[i] && has_sig[i] ? 1 : 0) | (key_ok[i] ? 2 : 0));
}

// Transaction::verify_signature, one lane per record (bzk_l1.cuh verify_one): k = SHA-512(R | A | signed form) with the signed form gathered in
// place from the uploaded record, then ed25519_verify_kernel's group equation with the same LDS columns.  Lanes whose record has no src or is
// Unsigned take their verdict from the parse flags and leave.
__global__ void __launch_bounds__(ED25519_BLOCK) l1_tx_verify_kernel(const uint8_t* __restrict__ data, const l1::L1Rec* __restrict__ rec, uint64_t n,
                                                                     const uint32_t* __restrict__ base_tab, uint8_t* __restrict__ ok) {
    __shared__ uint32_t lds[ed25519::LANE_WORDS * ED25519_BLOCK];
    const uint64_t i = (uint64_t)blockIdx.x * ED25519_BLOCK + threadIdx.x;
    if (i >= n) return;
    ok[i] = l1::verify_one(data, rec[i], base_tab, lds + threadIdx.x, ED25519_BLOCK);
}
// Transaction::hash, one lane per record (bzk_l1.cuh hash_one): SHA3-256 of the signed form.  A kernel of its own: Keccak's fifty state
// registers and four waves per block are not the verifier's profile.
__global__ void __launch_bounds__(SHA3_BLOCK) l1_tx_hash_kernel(const uint8_t* __restrict__ data, const l1::L1Rec* __restrict__ rec, uint64_t n,
                                                                uint32_t* __restrict__ digest) {
    const uint64_t i = (uint64_t)blockIdx.x * SHA3_BLOCK + threadIdx.x;
    if (i >= n) return;
    const keccak::Digest d = l1::hash_one(data, rec[i]);
#pragma unroll
    for (int k = 0; k < 8; ++k) digest[8 * i + k] = d.w[k];
}
// MerkleTree::new for the m trees of a call, whose node arrays lie one after another in `nodes` (tree[t].node_base, in nodes).
// Leaves first: one lane per leaf, leaf_start (m + 1 entries) says which tree a lane's leaf belongs to, merkle_leaf_map where it goes.
__global__ void __launch_bounds__(256) sha3_merkle_place_kernel(const uint32_t* __restrict__ leaves, const l1::TreeAt* __restrict__ tree,
                                                                const uint32_t* __restrict__ leaf_start, uint32_t m, uint32_t n_leaves,
                                                                uint32_t* __restrict__ nodes) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_leaves) return;
    const uint32_t t = l1::tree_of(leaf_start, m, i);
    const size_t at = (size_t)tree[t].node_base + l1::merkle_leaf_map(tree[t].len, i - leaf_start[t]);
#pragma unroll
    for (int w = 0; w < 8; ++w) nodes[8 * at + w] = leaves[8 * (size_t)i + w];
}
// Then one launch per level d, deepest first: one lane per parent over all trees (lane_start: m + 1 entries for this level; a tree shallower
// than d contributes no lanes).  64 bytes in, one Keccak permutation (bzk_l1.cuh merkle_parent_one).
__global__ void __launch_bounds__(SHA3_BLOCK) sha3_merkle_level_kernel(uint32_t* __restrict__ nodes, const l1::TreeAt* __restrict__ tree,
                                                                       const uint32_t* __restrict__ lane_start, uint32_t m, uint32_t d,
                                                                       uint32_t lanes) {
    const uint32_t i = blockIdx.x * SHA3_BLOCK + threadIdx.x;
    if (i >= lanes) return;
    const uint32_t t = l1::tree_of(lane_start, m, i);
    l1::merkle_parent_one(nodes + 8 * (size_t)tree[t].node_base, d, i - lane_start[t]);
}
// roots[t] = tree t's node 0; all_ok[t] (where tx_ok is given) = every record of body t verified
__global__ void __launch_bounds__(256) sha3_merkle_roots_kernel(const uint32_t* __restrict__ nodes, const l1::TreeAt* __restrict__ tree,
                                                                const uint32_t* __restrict__ leaf_start, const uint8_t* __restrict__ tx_ok, uint32_t m,
                                                                uint32_t* __restrict__ roots, uint8_t* __restrict__ all_ok) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
#pragma unroll
    for (int w = 0; w < 8; ++w) roots[8 * (size_t)t + w] = nodes[8 * (size_t)tree[t].node_base + w];
    if (tx_ok) {
        uint8_t all = 1;
        for (uint32_t i = leaf_start[t]; i < leaf_start[t + 1]; ++i) all &= tx_ok[i] ? 1 : 0;
        all_ok[t] = all;
    }
}

int32_t eddsa_table_dev(bzk_ctx* ctx, const Fr29** out) {
    if (!ctx->eddsa_tab) {
        std::vector<Fr29> tab;
        eddsa::base_table_build(tab);
        void* d = nullptr;
        BZK_HIP(ctx, hipMalloc(&d, tab.size() * sizeof(Fr29)));
        if (hipMemcpyAsync(d, tab.data(), tab.size() * sizeof(Fr29), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            (void)hipFree(d);
            ctx->last_error = "eddsa: table upload failed";
            return BZK_E_DEVICE;
        }
        ctx->eddsa_tab = d;
    }
    *out = (const Fr29*)ctx->eddsa_tab;
    return BZK_OK;
}

constexpr uint64_t EDDSA_LAUNCH_MAX = (uint64_t)1 << 24;  // signatures per launch
int32_t jubjub_verify_launch(bzk_ctx* ctx, const void* pub_xy_dev, const void* msg_dev, const void* sig_dev, uint64_t n, void* ok_dev) {
    if (n == 0) return BZK_OK;
    const void* pconsts;
    int rf, rp;
    BZK_TRY(poseidon_consts_dev_shared(ctx, 6, &pconsts, &rf, &rp));
    const Fr29* tab;
    BZK_TRY(eddsa_table_dev(ctx, &tab));
    return launch_rows(n, EDDSA_LAUNCH_MAX, EDDSA_BLOCK, [&](uint64_t off, uint64_t m, unsigned grid) {
        BZK_LAUNCH(ctx, "jubjub_verify", jubjub_verify_kernel, dim3(grid), dim3(EDDSA_BLOCK), 0, (const Fr*)pub_xy_dev + 2 * off,
                   (const Fr*)msg_dev + off, (const Fr*)sig_dev + 3 * off, m, (const Fr29*)pconsts, rf, rp, tab, (uint8_t*)ok_dev + off);
        return BZK_OK;
    });
}

int32_t jubjub_decompress_launch(bzk_ctx* ctx, const void* x_dev, const void* odd_dev, uint64_t n, void* xy_dev, void* ok_dev) {
    return launch_rows(n, EDDSA_LAUNCH_MAX, DECOMPRESS_BLOCK, [&](uint64_t off, uint64_t m, unsigned grid) {
        BZK_LAUNCH(ctx, "jubjub_decompress", jubjub_decompress_kernel, dim3(grid), dim3(DECOMPRESS_BLOCK), 0, (const Fr*)x_dev + off,
                   (const uint8_t*)odd_dev + off, m, (Fr*)xy_dev + 2 * off, (uint8_t*)ok_dev + off);
        return BZK_OK;
    });
}

// MpnTransaction::verify_signature for n parsed transactions (TxSoA from wire.hip, parsed by host_bincode.h): per chunk one decompress launch over
// the 2 m keys (src keys first, so that their points are the verifier's key array as they stand), the hash inputs, the arity-7 Poseidon batch, the
// signature kernel, the verdicts.  No field arithmetic on the host.  639 bytes of workspace per transaction.
int32_t mpn_tx_verify_run(bzk_ctx* ctx, const TxSoA& t, uint64_t n, uint8_t* ok, uint8_t* hash_out, uint8_t* src_xy_out, uint8_t* dst_xy_out) {
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "mpn_tx_verify_run", n, MPN_TX_CHUNK);
    uint8_t *dkx, *dodd, *dxy, *dkok, *dtok, *dnums, *dsig, *dtup, *dmsg, *dfit, *dver, *dok;
    // both keys of every transaction: the m src keys, then the m dst keys
    st.in(dkx, t.src_x, 32, 2); st.in_part(dkx, t.dst_x, 32, 1); st.in(dodd, t.src_odd, 1, 2); st.in_part(dodd, t.dst_odd, 1, 1);
    st.out(dxy, src_xy_out, 64, 2); st.out_part(dxy, dst_xy_out, 64, 1); st.scratch(dkok, 2);
    st.in(dtok, t.tok, 64); st.in(dnums, t.nums, 24); st.in(dsig, t.sig, 96); st.scratch(dtup, 224); st.out(dmsg, hash_out, 32);
    st.scratch(dfit, 1); st.scratch(dver, 1); st.out(dok, ok, 1);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t, uint64_t m) {
        BZK_TRY(jubjub_decompress_launch(ctx, dkx, dodd, 2 * m, dxy, dkok));
        const dim3 grid((unsigned)((m + 255) / 256));
        BZK_LAUNCH(ctx, "mpn_tx_tuple", mpn_tx_tuple_kernel, grid, dim3(256), 0, (const uint64_t*)dnums, (const Fr*)dtok, (const Fr*)(dxy + m * 64),
                   dkok + m, m, (Fr*)dtup, dfit);
        BZK_TRY(poseidon_launch(ctx, dtup, 7, m, dmsg));
        BZK_TRY(jubjub_verify_launch(ctx, dxy, dmsg, dsig, m, dver));
        BZK_LAUNCH(ctx, "mpn_tx_verdict", mpn_tx_verdict_kernel, grid, dim3(256), 0, dver, dkok, dfit, m, (Fr*)dmsg, dok);
        return BZK_OK;
    });
}

int32_t sha3_256_launch(bzk_ctx* ctx, const void* data_dev, const void* begin_dev, const void* end_dev, uint64_t base, const void* blank_dev,
                        uint64_t n, void* digest_dev, void* scalar_dev) {
    return launch_rows(n, EDDSA_LAUNCH_MAX, SHA3_BLOCK, [&](uint64_t off, uint64_t m, unsigned grid) {
        BZK_LAUNCH(ctx, "sha3_256", sha3_256_kernel, dim3(grid), dim3(SHA3_BLOCK), 0, (const uint8_t*)data_dev, (const uint64_t*)begin_dev + off,
                   (const uint64_t*)end_dev + off, base, blank_dev ? (const uint32_t*)blank_dev + off : nullptr, m,
                   digest_dev ? (uint32_t*)digest_dev + 8 * off : nullptr, scalar_dev ? (Fr*)scalar_dev + off : nullptr);
        return BZK_OK;
    });
}

// MpnWithdraw::verify_signature and verify_calldata for n parsed records (WdSoA from wire.hip, parsed by host_bincode.h).  A chunk ends at
// MPN_TX_CHUNK records or MPN_WD_CHUNK_BYTES of payment bytes, whichever comes first (a payment is at most MPN_WD_PAYMENT_MAX bytes, so a chunk
// always holds a record); its records' bytes go up as they stand, headers included, and the kernels index the payments inside them.  Per chunk:
// fingerprints (SHA3 with the calldata blanked, then ZkScalar::new), one decompress launch, the hash inputs, H2, H6, the signature kernel, the
// verdicts.  No hashing and no field arithmetic on the host.
int32_t mpn_withdraw_verify_run(bzk_ctx* ctx, const WdSoA& t, uint64_t n, uint8_t* ok, uint8_t* fp_out, uint8_t* xy_out) {
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "mpn_withdraw_verify_run", n, MPN_TX_CHUNK, MPN_WD_CHUNK_BYTES, [&](uint64_t i) { return (uint64_t)t.pay_len[i]; }, t.rec_off);
    std::vector<uint64_t> begin = round_bases(st.round_at, t.rec_off), end(n);  // payment ranges relative to their chunk's first byte
    for (uint64_t i = 0; i < n; ++i) {
        begin[i] = t.pay_off[i] - begin[i];
        end[i] = begin[i] + t.pay_len[i];
    }
    uint8_t *dbytes, *dbeg, *dend, *dcd, *dnonce, *dkx, *dfp, *dmsg, *dcall, *dxy, *dh2, *dsig, *dh6, *dodd, *dkok, *dfit, *dver, *dok;
    st.bytes(dbytes, t.txs, 0, 0); st.in(dbeg, begin.data(), 8); st.in(dend, end.data(), 8); st.in(dcd, t.cd_off, 4); st.in(dnonce, t.nonce, 4);
    st.in(dkx, t.key_x, 32); st.out(dfp, fp_out, 32); st.scratch(dmsg, 32); st.scratch(dcall, 32);
    st.out(dxy, xy_out, 64); st.scratch(dh2, 64); st.in(dsig, t.sig, 96); st.scratch(dh6, 192);
    st.in(dodd, t.key_odd, 1); st.scratch(dkok, 1); st.scratch(dfit, 1); st.scratch(dver, 1); st.out(dok, ok, 1);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t, uint64_t m) {
        BZK_TRY(sha3_256_launch(ctx, dbytes, dbeg, dend, 0, dcd, m, nullptr, dfp));
        BZK_TRY(jubjub_decompress_launch(ctx, dkx, dodd, m, dxy, dkok));
        const dim3 grid((unsigned)((m + 255) / 256));
        BZK_LAUNCH(ctx, "mpn_withdraw_inputs", mpn_withdraw_inputs_kernel, grid, dim3(256), 0, (const Fr*)dfp, (const uint32_t*)dnonce, (const Fr*)dxy,
                   dkok, (const Fr*)dsig, m, (Fr*)dh2, (Fr*)dh6, dfit);
        BZK_TRY(poseidon_launch(ctx, dh2, 2, m, dmsg));
        BZK_TRY(poseidon_launch(ctx, dh6, 6, m, dcall));
        BZK_TRY(jubjub_verify_launch(ctx, dxy, dmsg, dsig, m, dver));
        BZK_LAUNCH(ctx, "mpn_withdraw_verdict", mpn_withdraw_verdict_kernel, grid, dim3(256), 0, dver, dfit, (const Fr*)dcall, dbytes,
                   (const uint64_t*)dbeg, (const uint32_t*)dcd, m, dok);
        return BZK_OK;
    });
}

int32_t ed25519_table_dev(bzk_ctx* ctx, const uint32_t** out) {
    if (!ctx->ed25519_tab) {
        void* d = nullptr;
        BZK_HIP(ctx, hipMalloc(&d, ed25519::BASE_TAB_WORDS * 4));
        if (hipMemcpyAsync(d, ed25519::base_table_host(), ed25519::BASE_TAB_WORDS * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            (void)hipFree(d);
            ctx->last_error = "ed25519: table upload failed";
            return BZK_E_DEVICE;
        }
        ctx->ed25519_tab = d;
    }
    *out = (const uint32_t*)ctx->ed25519_tab;
    return BZK_OK;
}

static int32_t sha512_launch(bzk_ctx* ctx, const void* data_dev, const void* begin_dev, const void* end_dev, uint64_t base, uint64_t n,
                             void* digest_dev) {
    return launch_rows(n, EDDSA_LAUNCH_MAX, SHA512_BLOCK, [&](uint64_t off, uint64_t m, unsigned grid) {
        BZK_LAUNCH(ctx, "sha512", sha512_kernel, dim3(grid), dim3(SHA512_BLOCK), 0, (const uint8_t*)data_dev, (const uint64_t*)begin_dev + off,
                   (const uint64_t*)end_dev + off, base, m, (uint32_t*)digest_dev + 16 * off);
        return BZK_OK;
    });
}
// pk_at_dev / sig_at_dev null: keys and signatures are packed arrays
static int32_t ed25519_verify_launch(bzk_ctx* ctx, const void* pk_dev, const void* pk_at_dev, const void* sig_dev, const void* sig_at_dev,
                                     const void* data_dev, const void* begin_dev, const void* end_dev, uint64_t base, int32_t tail, uint64_t n,
                                     void* ok_dev) {
    if (n == 0) return BZK_OK;
    const uint32_t* tab;
    BZK_TRY(ed25519_table_dev(ctx, &tab));
    return launch_rows(n, EDDSA_LAUNCH_MAX, ED25519_BLOCK, [&](uint64_t off, uint64_t m, unsigned grid) {
        BZK_LAUNCH(ctx, "ed25519_verify", ed25519_verify_kernel, dim3(grid), dim3(ED25519_BLOCK), 0,
                   (const uint8_t*)pk_dev + (pk_at_dev ? 0 : 32 * off), pk_at_dev ? (const uint64_t*)pk_at_dev + off : nullptr,
                   (const uint8_t*)sig_dev + (sig_at_dev ? 0 : 64 * off), sig_at_dev ? (const uint64_t*)sig_at_dev + off : nullptr,
                   (const uint8_t*)data_dev, (const uint64_t*)begin_dev + off, (const uint64_t*)end_dev + off, base, tail, m, tab,
                   (uint8_t*)ok_dev + off);
        return BZK_OK;
    });
}

uint8_t mpn_deposit_sig_host(const DpSoA& t, uint64_t i) {
    if (!t.has_sig[i]) return 0;
    const uint8_t* pay = t.txs + t.pay_off[i];
    sha512::Msg body = sha512::msg_one(pay, t.tag_off[i]);
    body.tail = 0;  // the None tag of the unsigned form
    return ed25519::verify_host(pay + t.src_off[i], pay + t.sig_off[i], body);
}

// ContractDeposit::verify_signature and the address decompression for n parsed MpnDeposits (DpSoA from wire.hip, parsed by host_bincode.h).  Chunks
// as mpn_withdraw_verify_run cuts them; a chunk's records go up as they stand and the verifier reads key, signature and signed bytes inside them.
// Per chunk: one Ed25519 launch, one decompress launch, the verdicts.  No hashing and no field arithmetic on the host.
int32_t mpn_deposit_verify_run(bzk_ctx* ctx, const DpSoA& t, uint64_t n, uint8_t* ok, uint8_t* xy_out) {
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "mpn_deposit_verify_run", n, MPN_TX_CHUNK, MPN_WD_CHUNK_BYTES, [&](uint64_t i) { return t.rec_off[i + 1] - t.pay_off[i]; },
                        t.rec_off);
    std::vector<uint64_t> begin = round_bases(st.round_at, t.rec_off), end(n), pk_at(n), sig_at(n);  // relative to their chunk's first byte
    for (uint64_t i = 0; i < n; ++i) {
        begin[i] = t.pay_off[i] - begin[i];
        end[i] = begin[i] + t.tag_off[i];
        pk_at[i] = begin[i] + t.src_off[i];
        sig_at[i] = begin[i] + t.sig_off[i];
    }
    uint8_t *dbytes, *dbeg, *dend, *dpk, *dsg, *dkx, *dxy, *dodd, *dhas, *dkok, *dver, *dok;
    st.bytes(dbytes, t.txs, 0, 0); st.in(dbeg, begin.data(), 8); st.in(dend, end.data(), 8); st.in(dpk, pk_at.data(), 8); st.in(dsg, sig_at.data(), 8);
    st.in(dkx, t.key_x, 32); st.out(dxy, xy_out, 64); st.in(dodd, t.key_odd, 1); st.in(dhas, t.has_sig, 1); st.scratch(dkok, 1); st.scratch(dver, 1);
    st.out(dok, ok, 1);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t, uint64_t m) {
        BZK_TRY(ed25519_verify_launch(ctx, dbytes, dpk, dbytes, dsg, dbytes, dbeg, dend, 0, 0, m, dver));
        BZK_TRY(jubjub_decompress_launch(ctx, dkx, dodd, m, dxy, dkok));
        BZK_LAUNCH(ctx, "mpn_deposit_verdict", mpn_deposit_verdict_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, dver, dhas, dkok, m, dok);
        return BZK_OK;
    });
}

// the rounds of a host batch of messages: at most 2^20 messages or 64 MiB each, and at least one message
constexpr uint64_t MSG_ROUND = (uint64_t)1 << 20, MSG_ROUND_BYTES = (uint64_t)64 << 20;

// ---- wire-form L1 transactions and the block root (bzk_l1.cuh) -------------------------------------------------------------------------------
// The layout of a call's m trees: where each tree's nodes and leaves lie and, per level, which lanes are whose.  Host arithmetic only.
struct MerklePlan {
    std::vector<l1::TreeAt> tree;      // m
    std::vector<uint32_t> start;       // (depth + 1) rows of m + 1: row 0 the leaves' prefix sums, row d level d's lanes'
    uint32_t m = 0, depth = 0, n_leaves = 0, n_nodes = 0;
    const uint32_t* row(uint32_t d) const { return start.data() + (size_t)d * (m + 1); }
    bool build(const uint64_t* count, uint64_t trees) {
        uint64_t leaves = 0, nodes = 0;
        for (uint64_t t = 0; t < trees; ++t) {
            if (count[t] >= ((uint64_t)1 << 30)) return false;
            leaves += count[t];
            nodes += count[t] ? 2 * count[t] - 1 : 1;
        }
        if (trees >= ((uint64_t)1 << 31) || nodes >= ((uint64_t)1 << 31)) return false;  // node indices are 32-bit
        m = (uint32_t)trees; n_leaves = (uint32_t)leaves; n_nodes = (uint32_t)nodes;
        tree.resize(m);
        depth = 0;
        uint32_t at = 0;
        for (uint32_t t = 0; t < m; ++t) {
            tree[t] = {at, count[t] ? (uint32_t)(2 * count[t] - 1) : 1u};
            at += tree[t].len;
            depth = std::max(depth, l1::merkle_depth(tree[t].len));
        }
        start.assign((size_t)(depth + 1) * (m + 1), 0);
        for (uint32_t t = 0; t < m; ++t) {
            start[t + 1] = start[t] + (uint32_t)count[t];
            for (uint32_t d = 1; d <= depth; ++d) {
                uint32_t* r = start.data() + (size_t)d * (m + 1);
                r[t + 1] = r[t] + (d <= l1::merkle_depth(tree[t].len) ? l1::merkle_level_pairs(tree[t].len, d) : 0);
            }
        }
        return true;
    }
};
// leaves_dev (n_leaves x 32) -> nodes_dev (n_nodes x 32), roots_dev (m x 32) and, where tx_ok_dev is given, all_ok_dev (m); dtree / dstart: the
// plan's two arrays on the device.  Enqueues on the context's stream.
static int32_t merkle_enqueue(bzk_ctx* ctx, const MerklePlan& P, const void* leaves_dev, const void* tx_ok_dev, l1::TreeAt* dtree, uint32_t* dstart,
                              void* nodes_dev, void* roots_dev, void* all_ok_dev) {
    if (P.m == 0) return BZK_OK;
    BZK_HIP(ctx, hipMemcpyAsync(dtree, P.tree.data(), P.tree.size() * sizeof(l1::TreeAt), hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipMemcpyAsync(dstart, P.start.data(), P.start.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipMemsetAsync(nodes_dev, 0, (size_t)P.n_nodes * 32, ctx->stream));  // the node of a tree without leaves stays zero
    if (P.n_leaves)
        BZK_LAUNCH(ctx, "sha3_merkle_place", sha3_merkle_place_kernel, dim3((P.n_leaves + 255) / 256), dim3(256), 0, (const uint32_t*)leaves_dev,
                   (const l1::TreeAt*)dtree, (const uint32_t*)dstart, P.m, P.n_leaves, (uint32_t*)nodes_dev);
    for (uint32_t d = P.depth; d >= 1; --d) {
        const uint32_t lanes = P.row(d)[P.m];
        if (!lanes) continue;
        BZK_LAUNCH(ctx, "sha3_merkle_level", sha3_merkle_level_kernel, dim3((lanes + SHA3_BLOCK - 1) / SHA3_BLOCK), dim3(SHA3_BLOCK), 0,
                   (uint32_t*)nodes_dev, (const l1::TreeAt*)dtree, (const uint32_t*)(dstart + (size_t)d * (P.m + 1)), P.m, d, lanes);
    }
    BZK_LAUNCH(ctx, "sha3_merkle_roots", sha3_merkle_roots_kernel, dim3((P.m + 255) / 256), dim3(256), 0, (const uint32_t*)nodes_dev,
               (const l1::TreeAt*)dtree, (const uint32_t*)dstart, (const uint8_t*)tx_ok_dev, P.m, (uint32_t*)roots_dev, (uint8_t*)all_ok_dev);
    return BZK_OK;
}
// the same on host threads: nodes (n_nodes x 32) is the caller's
static void merkle_host(int threads, const MerklePlan& P, const uint8_t* leaves, const uint8_t* tx_ok, uint32_t* nodes, uint8_t* roots, uint8_t* all_ok) {
    memset(nodes, 0, (size_t)P.n_nodes * 32);
    host_for_each(P.n_leaves, threads, [&](uint64_t i) {
        const uint32_t t = l1::tree_of(P.row(0), P.m, (uint32_t)i);
        memcpy(nodes + 8 * ((size_t)P.tree[t].node_base + l1::merkle_leaf_map(P.tree[t].len, (uint32_t)i - P.row(0)[t])), leaves + 32 * i, 32);
    });
    for (uint32_t d = P.depth; d >= 1; --d) {
        const uint32_t* row = P.row(d);
        host_for_each(row[P.m], threads, [&](uint64_t i) {
            const uint32_t t = l1::tree_of(row, P.m, (uint32_t)i);
            l1::merkle_parent_one(nodes + 8 * (size_t)P.tree[t].node_base, d, (uint32_t)i - row[t]);
        });
    }
    for (uint32_t t = 0; t < P.m; ++t) {
        memcpy(roots + 32 * (size_t)t, nodes + 8 * (size_t)P.tree[t].node_base, 32);
        if (tx_ok) {
            uint8_t all = 1;
            for (uint32_t i = P.row(0)[t]; i < P.row(0)[t + 1]; ++i) all &= tx_ok[i] ? 1 : 0;
            all_ok[t] = all;
        }
    }
}

int32_t l1_check_host(int threads, const L1SoA& t, uint64_t n, const uint64_t* count, uint64_t m, uint8_t* ok, uint8_t* hash_out,
                      uint8_t* sig_ok_out, uint8_t* root_out) {
    MerklePlan P;
    if (count && !P.build(count, m)) return BZK_E_ARG;
    std::vector<uint8_t> hashes, verdicts;
    if (count && !hash_out) {
        hashes.resize(n * 32);
        hash_out = hashes.data();
    }
    if (!ok) {
        verdicts.resize(n);
        ok = verdicts.data();
    }
    const uint32_t* tab = ed25519::base_table_host();
    host_for_each(n, threads, [&](uint64_t i) {
        uint32_t lane[ed25519::LANE_WORDS];
        ok[i] = l1::verify_one(t.txs + t.rec_off[i], t.rec[i], tab, lane, 1);  // rec.at is 0: the record's own first byte is the base
        if (hash_out) {
            const keccak::Digest d = l1::hash_one(t.txs + t.rec_off[i], t.rec[i]);
            memcpy(hash_out + 32 * i, d.w, 32);
        }
    });
    if (count && m) {
        std::vector<uint32_t> nodes((size_t)P.n_nodes * 8);
        merkle_host(threads, P, hash_out, ok, nodes.data(), root_out, sig_ok_out);
    }
    return BZK_OK;
}

// Rounds end at l1::CHUNK records or l1::CHUNK_BYTES of record bytes (a record is at most l1::RECORD_MAX bytes, so a round always holds one); a
// round's records go up as they stand with their L1Rec, one verify launch and one hash launch per round.  Verdicts and hashes of all rounds stay
// on the device; with count given the trees are built from them there.
int32_t l1_check_run(bzk_ctx* ctx, const L1SoA& t, uint64_t n, const uint64_t* count, uint64_t m, uint8_t* ok, uint8_t* hash_out,
                     uint8_t* sig_ok_out, uint8_t* root_out) {
    if (n == 0 && (!count || m == 0)) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    MerklePlan P;
    if (count && !P.build(count, m)) return BZK_E_ARG;
    const std::vector<uint64_t> chunk_at = cut_rounds(n, l1::CHUNK, l1::CHUNK_BYTES, lengths(t.rec_off));
    const auto [cap, cap_bytes] = round_caps(chunk_at, t.rec_off);
    const bool want_hash = hash_out || count;
    WsLayout ws("l1_check_run");
    uint8_t *dbytes, *dok, *dhash, *dnodes, *droots, *dall;
    l1::L1Rec* drec;
    l1::TreeAt* dtree;
    uint32_t* dstart;
    ws.take(dbytes, cap_bytes + 8); ws.take(drec, cap ? cap : 1); ws.take(dok, n ? n : 1); ws.take(dhash, want_hash ? n * 32 + 32 : 32);
    ws.take(dnodes, (size_t)P.n_nodes * 32 + 32); ws.take(droots, (size_t)P.m * 32 + 32); ws.take(dall, (size_t)P.m + 1);
    ws.take(dtree, (size_t)P.m + 1); ws.take(dstart, P.start.size() + 1);
    BZK_TRY(ws.commit(ctx));
    const uint32_t* tab = nullptr;
    if (n) BZK_TRY(ed25519_table_dev(ctx, &tab));
    std::vector<l1::L1Rec> recs(cap);
    for (size_t c = 0; c + 1 < chunk_at.size(); ++c) {  // one stream: a round's uploads follow the previous round's kernels
        const uint64_t off = chunk_at[c], k = chunk_at[c + 1] - off;
        if (c) BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // recs is reused: the previous round's upload has to have left it
        for (uint64_t i = 0; i < k; ++i) {
            recs[i] = t.rec[off + i];
            recs[i].at = (uint32_t)(t.rec_off[off + i] - t.rec_off[off]);
        }
        BZK_HIP(ctx, hipMemcpyAsync(dbytes, t.txs + t.rec_off[off], t.rec_off[off + k] - t.rec_off[off], hipMemcpyHostToDevice, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(drec, recs.data(), k * sizeof(l1::L1Rec), hipMemcpyHostToDevice, ctx->stream));
        BZK_LAUNCH(ctx, "l1_tx_verify", l1_tx_verify_kernel, dim3((unsigned)((k + ED25519_BLOCK - 1) / ED25519_BLOCK)), dim3(ED25519_BLOCK), 0,
                   (const uint8_t*)dbytes, (const l1::L1Rec*)drec, k, tab, dok + off);
        if (want_hash)
            BZK_LAUNCH(ctx, "l1_tx_hash", l1_tx_hash_kernel, dim3((unsigned)((k + SHA3_BLOCK - 1) / SHA3_BLOCK)), dim3(SHA3_BLOCK), 0,
                       (const uint8_t*)dbytes, (const l1::L1Rec*)drec, k, (uint32_t*)dhash + 8 * off);
    }
    if (count && m) {
        BZK_TRY(merkle_enqueue(ctx, P, dhash, dok, dtree, dstart, dnodes, droots, dall));
        BZK_HIP(ctx, hipMemcpyAsync(root_out, droots, (size_t)P.m * 32, hipMemcpyDeviceToHost, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(sig_ok_out, dall, P.m, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (n && ok) BZK_HIP(ctx, hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, ctx->stream));
    if (n && hash_out) BZK_HIP(ctx, hipMemcpyAsync(hash_out, dhash, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BZK_OK;
}

}  // namespace bzk

using namespace bzk;

extern "C" {

int32_t bzk_jubjub_verify_batch_dev(bzk_ctx* ctx, const void* pub_xy_dev, const void* msg_dev, const void* sig_dev, uint64_t n, void* ok_dev) {
    if (!ctx || (n && (!pub_xy_dev || !msg_dev || !sig_dev || !ok_dev))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    return jubjub_verify_launch(ctx, pub_xy_dev, msg_dev, sig_dev, n, ok_dev);
}

int32_t bzk_jubjub_verify_batch(bzk_ctx* ctx, const uint8_t* pub_xy, const uint8_t* msg, const uint8_t* sig, uint64_t n, uint8_t* ok) {
    if (!ctx || (n && (!pub_xy || !msg || !sig || !ok))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_jubjub_verify_batch", n, (uint64_t)1 << 20);  // 193 bytes per signature: at most 193 MB of workspace
    uint8_t *dpub, *dmsg, *dsig, *dok;
    st.in(dpub, pub_xy, 64); st.in(dmsg, msg, 32); st.in(dsig, sig, 96); st.out(dok, ok, 1);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t, uint64_t m) { return jubjub_verify_launch(ctx, dpub, dmsg, dsig, m, dok); });
}

int32_t bzk_jubjub_decompress_batch_dev(bzk_ctx* ctx, const void* x_dev, const void* odd_dev, uint64_t n, void* xy_out_dev, void* ok_dev) {
    if (!ctx || (n && (!x_dev || !odd_dev || !xy_out_dev || !ok_dev))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    return jubjub_decompress_launch(ctx, x_dev, odd_dev, n, xy_out_dev, ok_dev);
}

int32_t bzk_jubjub_decompress_batch(bzk_ctx* ctx, const uint8_t* x, const uint8_t* odd, uint64_t n, uint8_t* xy_out, uint8_t* ok) {
    if (!ctx || (n && (!x || !odd || !xy_out || !ok))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_jubjub_decompress_batch", n, (uint64_t)1 << 20);  // 98 bytes per key
    uint8_t *dx, *dodd, *dxy, *dok;
    st.in(dx, x, 32); st.in(dodd, odd, 1); st.out(dxy, xy_out, 64); st.out(dok, ok, 1);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t, uint64_t m) { return jubjub_decompress_launch(ctx, dx, dodd, m, dxy, dok); });
}

// decompress, then verify: a key that does not decompress leaves (0, 0), which is off the curve, so the verifier's verdict is already 0.  The
// decompressed keys go through the context's workspace (65 bytes per key); its users are ordered by the context's stream
int32_t bzk_jubjub_verify_batch_compressed_dev(bzk_ctx* ctx, const void* pk_x_dev, const void* pk_odd_dev, const void* msg_dev, const void* sig_dev,
                                               uint64_t n, void* ok_dev) {
    if (!ctx || (n && (!pk_x_dev || !pk_odd_dev || !msg_dev || !sig_dev || !ok_dev))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    WsLayout ws("bzk_jubjub_verify_batch_compressed_dev");
    uint8_t *dxy, *dkok;
    ws.take(dxy, n * 64); ws.take(dkok, n);
    BZK_TRY(ws.commit(ctx));
    BZK_TRY(jubjub_decompress_launch(ctx, pk_x_dev, pk_odd_dev, n, dxy, dkok));
    return jubjub_verify_launch(ctx, dxy, msg_dev, sig_dev, n, ok_dev);
}

int32_t bzk_jubjub_verify_batch_compressed(bzk_ctx* ctx, const uint8_t* pk_x, const uint8_t* pk_odd, const uint8_t* msg, const uint8_t* sig, uint64_t n,
                                           uint8_t* ok) {
    if (!ctx || (n && (!pk_x || !pk_odd || !msg || !sig || !ok))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_jubjub_verify_batch_compressed", n, (uint64_t)1 << 20);  // 227 bytes per signature
    uint8_t *dx, *dodd, *dxy, *dkok, *dmsg, *dsig, *dok;
    st.in(dx, pk_x, 32); st.in(dodd, pk_odd, 1); st.scratch(dxy, 64); st.scratch(dkok, 1);
    st.in(dmsg, msg, 32); st.in(dsig, sig, 96); st.out(dok, ok, 1);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t, uint64_t m) {
        BZK_TRY(jubjub_decompress_launch(ctx, dx, dodd, m, dxy, dkok));
        return jubjub_verify_launch(ctx, dxy, dmsg, dsig, m, dok);
    });
}

int32_t bzk_sha3_256_batch_dev(bzk_ctx* ctx, const void* data_dev, const void* off_dev, uint64_t n, void* digest_out_dev, void* scalar_out_dev) {
    if (!ctx || (n && (!data_dev || !off_dev || (!digest_out_dev && !scalar_out_dev)))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    return sha3_256_launch(ctx, data_dev, off_dev, (const uint64_t*)off_dev + 1, 0, nullptr, n, digest_out_dev, scalar_out_dev);
}

int32_t bzk_sha3_256_batch(bzk_ctx* ctx, const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* digest_out, uint8_t* scalar_out) {
    if (!ctx || (n && (!data || !off || (!digest_out && !scalar_out)))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (!offsets_ok(off, n)) return BZK_E_ARG;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_sha3_256_batch", n, MSG_ROUND, MSG_ROUND_BYTES, lengths(off), off);
    uint8_t *ddata, *doff, *ddig, *dsc;
    st.bytes(ddata, data, 0, st.cap_bytes ? 0 : 1); st.offsets(doff); st.out(ddig, digest_out, 32); st.out(dsc, scalar_out, 32);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t a, uint64_t m) {
        return sha3_256_launch(ctx, ddata, doff, doff + 8, off[a], nullptr, m, digest_out ? ddig : nullptr, scalar_out ? dsc : nullptr);
    });
}

int32_t bzk_sha512_batch_dev(bzk_ctx* ctx, const void* data_dev, const void* off_dev, uint64_t n, void* digest_out_dev) {
    if (!ctx || (n && (!data_dev || !off_dev || !digest_out_dev))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    return sha512_launch(ctx, data_dev, off_dev, (const uint64_t*)off_dev + 1, 0, n, digest_out_dev);
}

int32_t bzk_sha512_batch(bzk_ctx* ctx, const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* digest_out) {
    if (n && (!data || !off || !digest_out)) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (!offsets_ok(off, n)) return BZK_E_ARG;
    if (!ctx) {  // the same per-lane code on host threads
        host_for_each(n, host_default_threads(), [&](uint64_t i) {
            const sha512::Digest d = sha512::sha512_one(sha512::msg_one(data + off[i], off[i + 1] - off[i]));
            memcpy(digest_out + 64 * i, d.w, 64);
        });
        return BZK_OK;
    }
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_sha512_batch", n, MSG_ROUND, MSG_ROUND_BYTES, lengths(off), off);
    uint8_t *ddata, *doff, *ddig;
    st.bytes(ddata, data, 0, st.cap_bytes ? 0 : 1); st.offsets(doff); st.out(ddig, digest_out, 64);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t a, uint64_t m) { return sha512_launch(ctx, ddata, doff, doff + 8, off[a], m, ddig); });
}

int32_t bzk_ed25519_verify_batch_dev(bzk_ctx* ctx, const void* pk_dev, const void* msg_dev, const void* off_dev, const void* sig_dev, uint64_t n,
                                     void* ok_dev) {
    if (!ctx || (n && (!pk_dev || !msg_dev || !off_dev || !sig_dev || !ok_dev))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    return ed25519_verify_launch(ctx, pk_dev, nullptr, sig_dev, nullptr, msg_dev, off_dev, (const uint64_t*)off_dev + 1, 0, -1, n, ok_dev);
}

int32_t bzk_ed25519_verify_batch(bzk_ctx* ctx, const uint8_t* pk, const uint8_t* msg, const uint64_t* off, const uint8_t* sig, uint64_t n,
                                 uint8_t* ok) {
    if (n && (!pk || !msg || !off || !sig || !ok)) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (!offsets_ok(off, n)) return BZK_E_ARG;
    if (!ctx) {
        host_for_each(n, host_default_threads(), [&](uint64_t i) {
            ok[i] = ed25519::verify_host(pk + 32 * i, sig + 64 * i, sha512::msg_one(msg + off[i], off[i + 1] - off[i]));
        });
        return BZK_OK;
    }
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_ed25519_verify_batch", n, MSG_ROUND, MSG_ROUND_BYTES, lengths(off), off);
    uint8_t *ddata, *doff, *dpk, *dsig, *dok;
    st.bytes(ddata, msg, 0, st.cap_bytes ? 0 : 1); st.offsets(doff); st.in(dpk, pk, 32); st.in(dsig, sig, 64); st.out(dok, ok, 1);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t a, uint64_t m) { return ed25519_verify_launch(ctx, dpk, nullptr, dsig, nullptr, ddata, doff, doff + 8, off[a], -1, m, dok); });
}

int32_t bzk_sha3_merkle_roots(bzk_ctx* ctx, const uint8_t* leaves, const uint64_t* count, uint64_t m, uint8_t* roots_out, uint8_t* nodes_out) {
    if (m && (!count || !roots_out)) return BZK_E_ARG;
    if (m == 0) return BZK_OK;
    MerklePlan P;
    if (!P.build(count, m) || (P.n_leaves && !leaves)) return BZK_E_ARG;
    if (!ctx) {  // the same per-lane code on host threads
        std::vector<uint32_t> own;
        if (!nodes_out || ((uintptr_t)nodes_out & 3)) own.resize((size_t)P.n_nodes * 8);
        uint32_t* nodes = own.empty() ? (uint32_t*)nodes_out : own.data();
        merkle_host(host_default_threads(), P, leaves, nullptr, nodes, roots_out, nullptr);
        if (nodes_out && !own.empty()) memcpy(nodes_out, nodes, (size_t)P.n_nodes * 32);
        return BZK_OK;
    }
    (void)hipSetDevice(ctx->device);
    WsLayout ws("bzk_sha3_merkle_roots");
    uint8_t *dleaves, *dnodes, *droots;
    l1::TreeAt* dtree;
    uint32_t* dstart;
    ws.take(dleaves, (size_t)P.n_leaves * 32 + 32); ws.take(dnodes, (size_t)P.n_nodes * 32); ws.take(droots, (size_t)P.m * 32);
    ws.take(dtree, P.m); ws.take(dstart, P.start.size());
    BZK_TRY(ws.commit(ctx));
    if (P.n_leaves) BZK_HIP(ctx, hipMemcpyAsync(dleaves, leaves, (size_t)P.n_leaves * 32, hipMemcpyHostToDevice, ctx->stream));
    BZK_TRY(merkle_enqueue(ctx, P, dleaves, nullptr, dtree, dstart, dnodes, droots, nullptr));
    BZK_HIP(ctx, hipMemcpyAsync(roots_out, droots, (size_t)P.m * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (nodes_out) BZK_HIP(ctx, hipMemcpyAsync(nodes_out, dnodes, (size_t)P.n_nodes * 32, hipMemcpyDeviceToHost, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BZK_OK;
}

int32_t bzk_sha3_merkle_roots_dev(bzk_ctx* ctx, const void* leaves_dev, const void* count_dev, uint64_t m, uint64_t n_leaves, void* roots_out_dev,
                                  void* nodes_out_dev) {
    if (!ctx || (m && (!count_dev || !roots_out_dev)) || (n_leaves && !leaves_dev)) return BZK_E_ARG;
    if (m == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    std::vector<uint64_t> count(m);  // the levels are laid out on the host: the counts come back first
    BZK_HIP(ctx, hipMemcpyAsync(count.data(), count_dev, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    MerklePlan P;
    if (!P.build(count.data(), m) || P.n_leaves != n_leaves) return BZK_E_ARG;
    WsLayout ws("bzk_sha3_merkle_roots_dev");
    uint8_t* dnodes;
    l1::TreeAt* dtree;
    uint32_t* dstart;
    ws.take(dnodes, nodes_out_dev ? 0 : (size_t)P.n_nodes * 32); ws.take(dtree, P.m); ws.take(dstart, P.start.size());
    BZK_TRY(ws.commit(ctx));
    BZK_TRY(merkle_enqueue(ctx, P, leaves_dev, nullptr, dtree, dstart, nodes_out_dev ? nodes_out_dev : dnodes, roots_out_dev, nullptr));
    // the plan's host arrays are read by the uploads just enqueued
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BZK_OK;
}

int32_t bzk_host_sha512(const uint8_t* in, uint64_t len, uint8_t out[64]) {
    if ((len && !in) || !out) return BZK_E_ARG;
    const uint8_t none = 0;
    const sha512::Digest d = sha512::sha512_one(sha512::msg_one(in ? in : &none, len));
    memcpy(out, d.w, 64);
    return BZK_OK;
}

int32_t bzk_host_ed25519_verify(const uint8_t pk[32], const uint8_t* msg, uint64_t len, const uint8_t sig[64]) {
    if (!pk || !sig || (len && !msg)) return BZK_E_ARG;
    const uint8_t none = 0;
    return ed25519::verify_host(pk, sig, sha512::msg_one(msg ? msg : &none, len));
}

}  // extern "C"
