// Batched Jubjub EdDSA key derivation and signing on the device (bzk_jubjub_keys_batch[_dev], bzk_jubjub_sign_batch[_dev], bzk_mpn_txs_sign):
// `JubJub::generate_keys` and `JubJub::sign` (src/crypto/jubjub/mod.rs:112-150) for n independent rows, one lane per row.  The arithmetic is
// bzk_eddsa_sign.cuh's keys_one and sign_one; this file holds the two kernels, the transaction signer's glue kernels and the entry points.  The
// table of multiples of BASE is the verifier's (eddsa.hip eddsa_table_dev).  ctx = NULL runs the same per-lane functions on host threads.

// as in eddsa.hip: the hashes share a kernel with the fixed-base walk, so their MDS matrix is re-read in every full round
#define BZK_POSEIDON_MDS_RELOAD 1
#include <mutex>

#include "bzk_decompress.cuh"
#include "bzk_eddsa_sign.cuh"
#include "bzk_internal.h"
#include "bzk_stage.h"
#include "host_bincode.h"
#include "host_mpn_world.h"  // g_work_error
#include "host_threads.h"

namespace bzk {

int32_t poseidon_consts_dev_shared(bzk_ctx* ctx, int t, const void** out, int* rf, int* rp);  // poseidon.hip
int32_t poseidon_consts_host29(int t, const Fr29** out, int* rf, int* rp);                    // poseidon.hip
int32_t poseidon_launch(bzk_ctx* ctx, const void* in_dev, uint32_t arity, uint64_t n, void* out_dev);  // poseidon.hip
int32_t eddsa_table_dev(bzk_ctx* ctx, const Fr29** out);                                      // eddsa.hip

// what a lane needs beside its own row: the two hashes' constants and the table of multiples of BASE
struct SignConsts {
    const Fr29 *c3, *c6, *tab;
    int rf3, rp3, rf6, rp6;
};

// One wave per block and no LDS: a signature is three dependent chains (hash, walk and inversion, hash) of some three thousand products, so
// the only parallelism is across lanes, and blocks of one wave spread a small batch over as many SIMDs as it has waves.
// gate (may be null): rows whose byte is 0 are not signed (zero signature, verdict 0)
constexpr int SIGN_BLOCK = 64;
__global__ void __launch_bounds__(SIGN_BLOCK) jubjub_sign_kernel(const Fr* __restrict__ keys, const Fr* __restrict__ msg, const uint8_t* __restrict__ gate,
                                                                 uint64_t n, SignConsts c, Fr* __restrict__ sig, uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * SIGN_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (gate && !gate[i]) {
        sig[3 * i] = sig[3 * i + 1] = sig[3 * i + 2] = Fr::zero();
        ok[i] = 0;
        return;
    }
    Fr s[3];
    ok[i] = eddsa::sign_one(keys + 4 * i, msg + i, c.c3, c.rf3, c.rp3, c.c6, c.rf6, c.rp6, c.tab, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) sig[3 * i + k] = s[k];
}

// Seed i = data[begin[i] - base .. end[i] - base).  Keccak's fifty state registers are dead before the walk starts; lanes of a wave leave the
// absorb loop at their own trip.
__global__ void __launch_bounds__(SIGN_BLOCK) jubjub_keys_kernel(const uint8_t* __restrict__ data, const uint64_t* __restrict__ begin,
                                                                 const uint64_t* __restrict__ end, uint64_t base, uint64_t n,
                                                                 const Fr29* __restrict__ tab, Fr* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * SIGN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = begin[i], e = end[i];
    Fr k[4];
    eddsa::keys_one(data + (b - base), e > b ? e - b : 0, tab, k);
#pragma unroll
    for (int j = 0; j < 4; ++j) keys[4 * i + j] = k[j];
}

// The hash inputs of m parsed transactions (bzk_decompress.cuh tx_tuple_one) and, per record, hfit = the hash can be computed (dst decompressed,
// token ids residues' limbs) and fit = hfit, the key's fields are residues' limbs and src is the compression of the key's pub
__global__ void __launch_bounds__(256) mpn_tx_sign_inputs_kernel(const uint64_t* __restrict__ nums, const Fr* __restrict__ tok,
                                                                 const Fr* __restrict__ dst_xy, const uint8_t* __restrict__ dst_ok,
                                                                 const Fr* __restrict__ src_x, const uint8_t* __restrict__ src_odd,
                                                                 const Fr* __restrict__ keys, uint64_t m, Fr* __restrict__ tuples,
                                                                 uint8_t* __restrict__ hfit, uint8_t* __restrict__ fit) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    Fr t[7];
    const bool h = eddsa::tx_tuple_one(nums + 3 * i, tok + 2 * i, dst_xy + 2 * i, dst_ok[i], t);
#pragma unroll
    for (int k = 0; k < 7; ++k) tuples[7 * i + k] = t[k];
    bool key_ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) key_ok = key_ok && eddsa::canonical(keys[4 * i + k]);
    hfit[i] = h ? 1 : 0;
    fit[i] = (h && key_ok && eddsa::compresses_to(keys + 4 * i, src_x[i], src_odd[i] != 0)) ? 1 : 0;
}
// the hash of a record whose hash could not be computed is zeros
__global__ void __launch_bounds__(256) mpn_tx_sign_hash_kernel(const uint8_t* __restrict__ hfit, uint64_t m, Fr* __restrict__ hash) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    if (!hfit[i]) hash[i] = Fr::zero();
}

constexpr uint64_t SIGN_LAUNCH_MAX = (uint64_t)1 << 24;  // rows per launch, as the verifier's
constexpr uint64_t SIGN_ROUND = (uint64_t)1 << 16;       // rows a host-pointer call stages per round: 257 bytes each, and the kernel's rate has levelled off
constexpr uint64_t KEYS_ROUND_BYTES = (uint64_t)64 << 20;

static int32_t sign_consts_dev(bzk_ctx* ctx, SignConsts& c) {
    const void *p3, *p6;
    BZK_TRY(poseidon_consts_dev_shared(ctx, 3, &p3, &c.rf3, &c.rp3));
    BZK_TRY(poseidon_consts_dev_shared(ctx, 6, &p6, &c.rf6, &c.rp6));
    c.c3 = (const Fr29*)p3;
    c.c6 = (const Fr29*)p6;
    return eddsa_table_dev(ctx, &c.tab);
}
// the same in host memory, with the width-8 constants of tx.hash(); built once
struct SignConstsHost {
    SignConsts c;
    const Fr29* c8;
    int rf8, rp8;
};
static int32_t sign_consts_host(SignConstsHost& h) {
    static std::once_flag once;
    static std::vector<Fr29> tab;
    std::call_once(once, [] { eddsa::base_table_build(tab); });
    BZK_TRY(poseidon_consts_host29(3, &h.c.c3, &h.c.rf3, &h.c.rp3));
    BZK_TRY(poseidon_consts_host29(6, &h.c.c6, &h.c.rf6, &h.c.rp6));
    BZK_TRY(poseidon_consts_host29(8, &h.c8, &h.rf8, &h.rp8));
    h.c.tab = tab.data();
    return BZK_OK;
}

static int32_t jubjub_sign_launch(bzk_ctx* ctx, const void* keys_dev, const void* msg_dev, const void* gate_dev, uint64_t n, void* sig_dev,
                                  void* ok_dev) {
    if (n == 0) return BZK_OK;
    SignConsts c;
    BZK_TRY(sign_consts_dev(ctx, c));
    return launch_rows(n, SIGN_LAUNCH_MAX, SIGN_BLOCK, [&](uint64_t off, uint64_t m, unsigned grid) {
        BZK_LAUNCH(ctx, "jubjub_sign", jubjub_sign_kernel, dim3(grid), dim3(SIGN_BLOCK), 0, (const Fr*)keys_dev + 4 * off, (const Fr*)msg_dev + off,
                   gate_dev ? (const uint8_t*)gate_dev + off : nullptr, m, c, (Fr*)sig_dev + 3 * off, (uint8_t*)ok_dev + off);
        return BZK_OK;
    });
}
static int32_t jubjub_keys_launch(bzk_ctx* ctx, const void* data_dev, const void* begin_dev, const void* end_dev, uint64_t base, uint64_t n,
                                  void* keys_dev) {
    if (n == 0) return BZK_OK;
    const Fr29* tab;
    BZK_TRY(eddsa_table_dev(ctx, &tab));
    return launch_rows(n, SIGN_LAUNCH_MAX, SIGN_BLOCK, [&](uint64_t off, uint64_t m, unsigned grid) {
        BZK_LAUNCH(ctx, "jubjub_keys", jubjub_keys_kernel, dim3(grid), dim3(SIGN_BLOCK), 0, (const uint8_t*)data_dev,
                   (const uint64_t*)begin_dev + off, (const uint64_t*)end_dev + off, base, m, tab, (Fr*)keys_dev + 4 * off);
        return BZK_OK;
    });
}

// one row on the host: bytes in, bytes out (the caller's buffers need no alignment)
static uint8_t sign_row_host(const SignConsts& c, const uint8_t* key, const uint8_t* msg, uint8_t* sig) {
    Fr k[4], m, s[3];
    memcpy(k, key, 128);
    memcpy(&m, msg, 32);
    const uint8_t ok = eddsa::sign_one(k, &m, c.c3, c.rf3, c.rp3, c.c6, c.rf6, c.rp6, c.tab, s);
    memcpy(sig, s, 96);
    return ok;
}

// MpnTransaction signing for n parsed transactions (TxParsed from host_bincode.h) and n keys: per round of MPN_TX_CHUNK records one decompress
// launch over the dst keys, the hash inputs and the two fitness bytes, the arity-7 Poseidon batch, the signing kernel gated by fit.  sig n x 96,
// ok n, hash_out n x 32 or null (host memory).  No field arithmetic on the host.  The staged key bytes are overwritten before the call returns.
static int32_t mpn_txs_sign_run(bzk_ctx* ctx, const TxSoA& t, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* ok, uint8_t* hash_out) {
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "mpn_txs_sign_run", n, MPN_TX_CHUNK);
    uint8_t *dkeys, *dsx, *ddx, *dsodd, *ddodd, *dxy, *dkok, *dtok, *dnums, *dtup, *dmsg, *dsig, *dhfit, *dfit, *dok;
    st.in(dkeys, keys, 128); st.in(dsx, t.src_x, 32); st.in(ddx, t.dst_x, 32); st.in(dsodd, t.src_odd, 1); st.in(ddodd, t.dst_odd, 1);
    st.scratch(dxy, 64); st.scratch(dkok, 1); st.in(dtok, t.tok, 64); st.in(dnums, t.nums, 24); st.scratch(dtup, 224);
    st.out(dmsg, hash_out, 32); st.out(dsig, sig, 96); st.scratch(dhfit, 1); st.scratch(dfit, 1); st.out(dok, ok, 1);
    st.wipe(dkeys, st.cap * 128);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t, uint64_t m) {
        BZK_TRY(jubjub_decompress_launch(ctx, ddx, ddodd, m, dxy, dkok));
        const dim3 grid((unsigned)((m + 255) / 256));
        BZK_LAUNCH(ctx, "mpn_tx_sign_inputs", mpn_tx_sign_inputs_kernel, grid, dim3(256), 0, (const uint64_t*)dnums, (const Fr*)dtok, (const Fr*)dxy,
                   (const uint8_t*)dkok, (const Fr*)dsx, (const uint8_t*)dsodd, (const Fr*)dkeys, m, (Fr*)dtup, dhfit, dfit);
        BZK_TRY(poseidon_launch(ctx, dtup, 7, m, dmsg));
        BZK_TRY(jubjub_sign_launch(ctx, dkeys, dmsg, dfit, m, dsig, dok));
        BZK_LAUNCH(ctx, "mpn_tx_sign_hash", mpn_tx_sign_hash_kernel, grid, dim3(256), 0, (const uint8_t*)dhfit, m, (Fr*)dmsg);
        return BZK_OK;
    });
}
// the same per-lane functions on host threads
static int32_t mpn_txs_sign_host(int threads, const TxParsed& P, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* ok, uint8_t* hash_out) {
    SignConstsHost h;
    BZK_TRY(sign_consts_host(h));
    host_for_each(n, threads, [&](uint64_t i) {
        Fr dx, sx, dxy[2], tok[2], k[4], tup[7], s[3];
        memcpy(&dx, &P.dst_x[32 * i], 32);
        memcpy(&sx, &P.src_x[32 * i], 32);
        memcpy(tok, &P.tok[64 * i], 64);
        memcpy(k, keys + 128 * i, 128);
        const uint8_t dst_ok = eddsa::decompress_one(dx, P.dst_odd[i] != 0, dxy);
        const bool hfit = eddsa::tx_tuple_one(&P.nums[3 * i], tok, dxy, dst_ok, tup);
        bool key_ok = true;
        for (int j = 0; j < 4; ++j) key_ok = key_ok && eddsa::canonical(k[j]);
        const bool fit = hfit && key_ok && eddsa::compresses_to(k, sx, P.src_odd[i] != 0);
        const Fr msg = hfit ? poseidon29_hash<8>(tup, h.c8, h.rf8, h.rp8) : Fr::zero();
        ok[i] = 0;
        memset(sig + 96 * i, 0, 96);
        if (fit) {
            ok[i] = eddsa::sign_one(k, &msg, h.c.c3, h.c.rf3, h.c.rp3, h.c.c6, h.c.rf6, h.c.rp6, h.c.tab, s);
            memcpy(sig + 96 * i, s, 96);
        }
        if (hash_out) memcpy(hash_out + 32 * i, &msg, 32);
    });
    return BZK_OK;
}

}  // namespace bzk

using namespace bzk;

extern "C" {

int32_t bzk_jubjub_sign_batch_dev(bzk_ctx* ctx, const void* keys_dev, const void* msg_dev, uint64_t n, void* sig_out_dev, void* ok_dev) {
    if (!ctx || (n && (!keys_dev || !msg_dev || !sig_out_dev || !ok_dev))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    return jubjub_sign_launch(ctx, keys_dev, msg_dev, nullptr, n, sig_out_dev, ok_dev);
}

int32_t bzk_jubjub_sign_batch(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* msg, uint64_t n, uint8_t* sig_out, uint8_t* ok) {
    if (n && (!keys || !msg || !sig_out || !ok)) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (!ctx) {  // the same per-lane code on host threads
        SignConstsHost h;
        BZK_TRY(sign_consts_host(h));
        host_for_each(n, host_default_threads(), [&](uint64_t i) { ok[i] = sign_row_host(h.c, keys + 128 * i, msg + 32 * i, sig_out + 96 * i); });
        return BZK_OK;
    }
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_jubjub_sign_batch", n, SIGN_ROUND);
    uint8_t *dkeys, *dmsg, *dsig, *dok;
    st.in(dkeys, keys, 128); st.in(dmsg, msg, 32); st.out(dsig, sig_out, 96); st.out(dok, ok, 1);
    st.wipe(dkeys, st.cap * 128);  // the staged keys do not outlive the call
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t, uint64_t m) { return jubjub_sign_launch(ctx, dkeys, dmsg, nullptr, m, dsig, dok); });
}

int32_t bzk_jubjub_keys_batch_dev(bzk_ctx* ctx, const void* seeds_dev, const void* off_dev, uint64_t n, void* keys_out_dev) {
    if (!ctx || (n && (!seeds_dev || !off_dev || !keys_out_dev))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    return jubjub_keys_launch(ctx, seeds_dev, off_dev, (const uint64_t*)off_dev + 1, 0, n, keys_out_dev);
}

int32_t bzk_jubjub_keys_batch(bzk_ctx* ctx, const uint8_t* seeds, const uint64_t* off, uint64_t n, uint8_t* keys_out) {
    if (n && (!off || !keys_out)) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (!offsets_ok(off, n) || (off[n] && !seeds)) return BZK_E_ARG;
    const uint8_t none = 0;
    if (!seeds) seeds = &none;  // n empty seeds
    if (!ctx) {  // the same per-lane code on host threads
        SignConstsHost h;
        BZK_TRY(sign_consts_host(h));
        host_for_each(n, host_default_threads(), [&](uint64_t i) {
            Fr k[4];
            eddsa::keys_one(seeds + off[i], off[i + 1] - off[i], h.c.tab, k);
            memcpy(keys_out + 128 * i, k, 128);
        });
        return BZK_OK;
    }
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_jubjub_keys_batch", n, SIGN_ROUND, KEYS_ROUND_BYTES, lengths(off), off);
    uint8_t *ddata, *doff, *dkeys;
    st.bytes(ddata, seeds, 0, 8); st.offsets(doff); st.out(dkeys, keys_out, 128);
    st.wipe(ddata, st.cap_bytes + 8); st.wipe(dkeys, st.cap * 128);  // neither the staged seeds nor the keys outlive the call
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t a, uint64_t m) { return jubjub_keys_launch(ctx, ddata, doff, doff + 8, off[a], m, dkeys); });
}

int32_t bzk_mpn_txs_sign(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* txs_out, uint8_t* ok,
                         uint8_t* hash_out) {
    if (n && (!keys || !txs || !txs_out || !ok)) return BZK_E_ARG;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        TxParsed P;
        if (!parse_txs(txs, len, n, P, g_work_error)) return BZK_E_ARG;
        std::vector<uint8_t> sig(n * 96);
        if (ctx) BZK_TRY(mpn_txs_sign_run(ctx, P.soa(), keys, n, sig.data(), ok, hash_out));
        else BZK_TRY(mpn_txs_sign_host(host_default_threads(), P, keys, n, sig.data(), ok, hash_out));
        if (txs_out != txs) memmove(txs_out, txs, len);
        for (uint64_t i = 0; i < n; ++i)
            if (ok[i]) memcpy(txs_out + P.rec_end[i] - 96, &sig[96 * i], 96);
        return BZK_OK;
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

}  // extern "C"
