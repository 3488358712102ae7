// Batched Ed25519 key derivation and signing on the device (bzk_ed25519_keys_batch[_dev], bzk_ed25519_sign_batch[_dev], and the signing stage of
// bzk_mpn_deposits_sign and bzk_l1_txs_sign, whose entry points are wire.hip's): `Ed25519::generate_keys` and `Ed25519::sign`
// (src/crypto/ed25519.rs:70-80) for n independent rows, one lane per row.  The arithmetic is bzk_ed25519_sign.cuh's keys_one and sign_one; this
// file holds the kernels and their orchestration.  The table of multiples of B is the verifier's (eddsa.hip ed25519_table_dev).  ctx = NULL runs
// the same per-lane functions on host threads.
#include "bzk_ed25519_sign.cuh"
#include "bzk_ed25519_sign.h"
#include "bzk_internal.h"
#include "bzk_l1.cuh"
#include "bzk_stage.h"
#include "host_threads.h"

namespace bzk {

// One wave per block and no LDS: a signature is a chain of two hashes, 64 dependent additions and an inversion, so the only parallelism is
// across lanes, and blocks of one wave spread a small batch over as many SIMDs as it has waves.  The nonce's nibbles come off the low end of a
// shifting register octet (base_mul_encode), so no LDS column is needed for them.
//
// Row i: key i = keys[64 i ..) (secret | public), message i = data[begin[i] - base .. end[i] - base) followed by the byte `tail` where
// tail >= 0.  exp: 64 bytes per row of this launch for a | prefix; sig: 64 bytes per row, where the lane stores R before it hashes R | A | M.
// src_at (may be null): the row is signed only where the 32 bytes at data[src_at[i]] equal the key's public half; else a zero row and ok = 0.
// ok may be null where src_at is.
constexpr int ED_SIGN_BLOCK = 64;
__global__ void __launch_bounds__(ED_SIGN_BLOCK) ed25519_sign_kernel(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ data,
                                                                     const uint64_t* __restrict__ begin, const uint64_t* __restrict__ end,
                                                                     const uint64_t* __restrict__ src_at, uint64_t base, int32_t tail, uint64_t n,
                                                                     const uint32_t* __restrict__ base_tab, uint8_t* exp, uint8_t* sig, uint8_t* ok) {
    const uint64_t i = (uint64_t)blockIdx.x * ED_SIGN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* key = keys + 64 * i;
    uint8_t* out = sig + 64 * i;
    if (src_at && !ed25519::bytes32_equal(data + src_at[i], key + 32)) {
        const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        ed25519::store_words8(out, zero);
        ed25519::store_words8(out + 32, zero);
        ok[i] = 0;
        return;
    }
    const uint64_t b = begin[i], e = end[i];
    sha512::Msg body = sha512::msg_one(data + (b - base), e > b ? e - b : 0);
    body.tail = tail;
    ed25519::expand_store(key, exp + 64 * i);
    ed25519::sign_one(exp + 64 * i, key + 32, body, body, base_tab, out);
    if (ok) ok[i] = 1;
}

// Seed i = data[begin[i] - base .. end[i] - base).  Keccak's fifty state registers are dead before SHA-512 and the walk start; lanes of a wave
// leave the absorb loop at their own trip.
__global__ void __launch_bounds__(ED_SIGN_BLOCK) ed25519_keys_kernel(const uint8_t* __restrict__ data, const uint64_t* __restrict__ begin,
                                                                     const uint64_t* __restrict__ end, uint64_t base, uint64_t n,
                                                                     const uint32_t* __restrict__ base_tab, uint8_t* keys) {
    const uint64_t i = (uint64_t)blockIdx.x * ED_SIGN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint64_t b = begin[i], e = end[i];
    ed25519::keys_one(data + (b - base), e > b ? e - b : 0, base_tab, keys + 64 * i);
}

// TxBuilder::sign_tx, one lane per record.  data: 128 bytes per record of this launch (a | prefix | R | s, the lane's own), then the records as
// they stand; rec[i].at counts from data.  Both hashes read the signed form in place as a gathered message whose first pieces are the lane's
// prefix, and R with the record's own src.  A record with no src, or whose src is not the key's public half, gets a zero row and ok = 0.
constexpr uint32_t L1_SIGN_HDR = 128;
__global__ void __launch_bounds__(ED_SIGN_BLOCK) l1_tx_sign_kernel(uint8_t* data, const l1::L1Rec* __restrict__ rec, const uint8_t* __restrict__ keys,
                                                                   uint64_t n, const uint32_t* __restrict__ base_tab, uint8_t* sig, uint8_t* ok) {
    const uint64_t i = (uint64_t)blockIdx.x * ED_SIGN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const l1::L1Rec r = rec[i];
    const uint8_t* key = keys + 64 * i;
    uint8_t* out = sig + 64 * i;
    if (!(r.flags & l1::HAS_SRC) || !ed25519::bytes32_equal(data + r.at + r.key_off, key + 32)) {
        const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        ed25519::store_words8(out, zero);
        ed25519::store_words8(out + 32, zero);
        ok[i] = 0;
        return;
    }
    const uint32_t hdr = L1_SIGN_HDR * (uint32_t)i;
    ed25519::expand_store(key, data + hdr);
    const gather::Msg body_r = ed25519::signed_form_prefixed(data, r.at, r.cut_a, r.cut_b, r.sig_tag, hdr + 32);
    const gather::Msg body_k = gather::signed_form<true>(data, r.at, r.cut_a, r.cut_b, r.sig_tag, hdr + 64 - r.at, r.key_off);  // R's offset wraps back
    ed25519::sign_one(data + hdr, data + r.at + r.key_off, body_r, body_k, base_tab, data + hdr + 64);
    uint32_t w[8];
    ed25519::load_words8(data + hdr + 64, w);
    ed25519::store_words8(out, w);
    ed25519::load_words8(data + hdr + 96, w);
    ed25519::store_words8(out + 32, w);
    ok[i] = 1;
}
// Transaction::hash of the same records (bzk_l1.cuh hash_one), as eddsa.hip's l1_tx_hash_kernel: Keccak's profile is not the signer's
__global__ void __launch_bounds__(256) l1_tx_sign_hash_kernel(const uint8_t* __restrict__ data, const l1::L1Rec* __restrict__ rec, uint64_t n,
                                                              uint32_t* __restrict__ digest) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const keccak::Digest d = l1::hash_one(data, rec[i]);
#pragma unroll
    for (int k = 0; k < 8; ++k) digest[8 * i + k] = d.w[k];
}

constexpr uint64_t ED_SIGN_LAUNCH_MAX = (uint64_t)1 << 24;  // rows per launch, as the verifier's

// exp_dev: 64 bytes for each of min(n, ED_SIGN_LAUNCH_MAX) rows; launches follow one another on the stream, so they share it
static int32_t ed25519_sign_launch(bzk_ctx* ctx, const void* keys_dev, const void* data_dev, const void* begin_dev, const void* end_dev,
                                   const void* src_at_dev, uint64_t base, int32_t tail, uint64_t n, void* exp_dev, void* sig_dev, void* ok_dev) {
    if (n == 0) return BZK_OK;
    const uint32_t* tab;
    BZK_TRY(ed25519_table_dev(ctx, &tab));
    return launch_rows(n, ED_SIGN_LAUNCH_MAX, ED_SIGN_BLOCK, [&](uint64_t off, uint64_t m, unsigned grid) {
        BZK_LAUNCH(ctx, "ed25519_sign", ed25519_sign_kernel, dim3(grid), dim3(ED_SIGN_BLOCK), 0, (const uint8_t*)keys_dev + 64 * off,
                   (const uint8_t*)data_dev, (const uint64_t*)begin_dev + off, (const uint64_t*)end_dev + off,
                   src_at_dev ? (const uint64_t*)src_at_dev + off : nullptr, base, tail, m, tab, (uint8_t*)exp_dev, (uint8_t*)sig_dev + 64 * off,
                   ok_dev ? (uint8_t*)ok_dev + off : nullptr);
        return BZK_OK;
    });
}
static int32_t ed25519_keys_launch(bzk_ctx* ctx, const void* data_dev, const void* begin_dev, const void* end_dev, uint64_t base, uint64_t n,
                                   void* keys_dev) {
    if (n == 0) return BZK_OK;
    const uint32_t* tab;
    BZK_TRY(ed25519_table_dev(ctx, &tab));
    return launch_rows(n, ED_SIGN_LAUNCH_MAX, ED_SIGN_BLOCK, [&](uint64_t off, uint64_t m, unsigned grid) {
        BZK_LAUNCH(ctx, "ed25519_keys", ed25519_keys_kernel, dim3(grid), dim3(ED_SIGN_BLOCK), 0, (const uint8_t*)data_dev,
                   (const uint64_t*)begin_dev + off, (const uint64_t*)end_dev + off, base, m, tab, (uint8_t*)keys_dev + 64 * off);
        return BZK_OK;
    });
}

// one row on the host: a | prefix on the stack, overwritten before it leaves
static void sign_row_host(const uint8_t* key, const sha512::Msg& body, uint8_t* sig) {
    uint8_t exp[ed25519::EXPANDED_BYTES];
    ed25519::expand_store(key, exp);
    ed25519::sign_one(exp, key + 32, body, body, ed25519::base_table_host(), sig);
    volatile uint8_t* v = exp;
    for (int k = 0; k < ed25519::EXPANDED_BYTES; ++k) v[k] = 0;
}

static int32_t mpn_deposits_sign_run(bzk_ctx* ctx, const DpSoA& t, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* ok) {
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "mpn_deposits_sign_run", n, ED25519_SIGN_ROUND, ED25519_SIGN_ROUND_BYTES,
                        lengths(t.rec_off), t.rec_off);
    std::vector<uint64_t> begin = round_bases(st.round_at, t.rec_off), end(n), src_at(n);  // relative to their round's first byte
    for (uint64_t i = 0; i < n; ++i) {
        begin[i] = t.pay_off[i] - begin[i];
        end[i] = begin[i] + t.tag_off[i];
        src_at[i] = begin[i] + t.src_off[i];
    }
    uint8_t *dbytes, *dbeg, *dend, *dsrc, *dkeys, *dexp, *dsig, *dok;
    st.bytes(dbytes, t.txs, 0, 0); st.in(dbeg, begin.data(), 8); st.in(dend, end.data(), 8); st.in(dsrc, src_at.data(), 8); st.in(dkeys, keys, 64);
    st.scratch(dexp, 64); st.out(dsig, sig, 64); st.out(dok, ok, 1);
    st.wipe(dkeys, st.cap * 64); st.wipe(dexp, st.cap * 64);  // neither the staged keys nor their expansions outlive the call
    BZK_TRY(st.ws.commit(ctx));
    // tail 0: the None tag of the unsigned form
    return st.run([&](uint64_t, uint64_t m) { return ed25519_sign_launch(ctx, dkeys, dbytes, dbeg, dend, dsrc, 0, 0, m, dexp, dsig, dok); });
}

int32_t mpn_deposits_sign_all(bzk_ctx* ctx, int threads, const DpSoA& t, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* ok) {
    if (ctx) return mpn_deposits_sign_run(ctx, t, keys, n, sig, ok);
    host_for_each(n, threads, [&](uint64_t i) {
        const uint8_t* pay = t.txs + t.pay_off[i];
        ok[i] = ed25519::bytes32_equal(pay + t.src_off[i], keys + 64 * i + 32) ? 1 : 0;
        memset(sig + 64 * i, 0, 64);
        if (!ok[i]) return;
        sha512::Msg body = sha512::msg_one(pay, t.tag_off[i]);
        body.tail = 0;
        sign_row_host(keys + 64 * i, body, sig + 64 * i);
    });
    return BZK_OK;
}

static int32_t l1_txs_sign_run(bzk_ctx* ctx, const L1SoA& t, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* ok, uint8_t* hash_out) {
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "l1_txs_sign_run", n, ED25519_SIGN_ROUND, ED25519_SIGN_ROUND_BYTES,
                        lengths(t.rec_off), t.rec_off);
    const uint64_t hdr_bytes = st.cap * L1_SIGN_HDR;  // at most 8 MiB in front of at most 64 MiB + one record: offsets stay far below 2^32
    const std::vector<uint64_t> base = round_bases(st.round_at, t.rec_off);
    std::vector<l1::L1Rec> recs(t.rec, t.rec + n);  // at: behind the lanes' headers, relative to the round's first byte
    for (uint64_t i = 0; i < n; ++i) recs[i].at = (uint32_t)(hdr_bytes + (t.rec_off[i] - base[i]));
    uint8_t *dbytes, *drec, *dkeys, *dsig, *dok, *dhash;
    st.bytes(dbytes, t.txs, hdr_bytes, 8); st.in(drec, recs.data(), sizeof(l1::L1Rec)); st.in(dkeys, keys, 64); st.out(dsig, sig, 64);
    st.out(dok, ok, 1);
    if (hash_out) st.out(dhash, hash_out, 32);
    else st.ws.take(dhash, 32);
    st.wipe(dkeys, st.cap * 64); st.wipe(dbytes, hdr_bytes);  // the staged keys and the lanes' a | prefix do not outlive the call
    BZK_TRY(st.ws.commit(ctx));
    const uint32_t* tab;
    BZK_TRY(ed25519_table_dev(ctx, &tab));
    return st.run([&](uint64_t, uint64_t m) {
        BZK_LAUNCH(ctx, "l1_tx_sign", l1_tx_sign_kernel, dim3((unsigned)((m + ED_SIGN_BLOCK - 1) / ED_SIGN_BLOCK)), dim3(ED_SIGN_BLOCK), 0, dbytes,
                   (const l1::L1Rec*)drec, (const uint8_t*)dkeys, m, tab, dsig, dok);
        if (hash_out)
            BZK_LAUNCH(ctx, "l1_tx_sign_hash", l1_tx_sign_hash_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (const uint8_t*)dbytes,
                       (const l1::L1Rec*)drec, m, (uint32_t*)dhash);
        return BZK_OK;
    });
}

int32_t l1_txs_sign_all(bzk_ctx* ctx, int threads, const L1SoA& t, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* ok, uint8_t* hash_out) {
    if (ctx) return l1_txs_sign_run(ctx, t, keys, n, sig, ok, hash_out);
    host_for_each(n, threads, [&](uint64_t i) {
        const uint8_t* rec = t.txs + t.rec_off[i];
        const l1::L1Rec& r = t.rec[i];  // at is 0: the record's own first byte is the base
        if (hash_out) {
            const keccak::Digest d = l1::hash_one(rec, r);
            memcpy(hash_out + 32 * i, d.w, 32);
        }
        ok[i] = ((r.flags & l1::HAS_SRC) && ed25519::bytes32_equal(rec + r.key_off, keys + 64 * i + 32)) ? 1 : 0;
        memset(sig + 64 * i, 0, 64);
        if (!ok[i]) return;
        // a gathered message has one base: the lane's 128 bytes and a copy of the record behind them, as the kernel's staging has them
        const uint64_t len = t.rec_off[i + 1] - t.rec_off[i];
        std::vector<uint8_t> buf(L1_SIGN_HDR + len + 8);
        memcpy(buf.data() + L1_SIGN_HDR, rec, len);
        uint8_t* data = buf.data();
        ed25519::expand_store(keys + 64 * i, data);
        const gather::Msg body_r = ed25519::signed_form_prefixed(data, L1_SIGN_HDR, r.cut_a, r.cut_b, r.sig_tag, 32);
        const gather::Msg body_k = gather::signed_form<true>(data, L1_SIGN_HDR, r.cut_a, r.cut_b, r.sig_tag, 64 - L1_SIGN_HDR, r.key_off);
        ed25519::sign_one(data, data + L1_SIGN_HDR + r.key_off, body_r, body_k, ed25519::base_table_host(), data + 64);
        memcpy(sig + 64 * i, data + 64, 64);
        volatile uint8_t* v = data;
        for (int k = 0; k < ed25519::EXPANDED_BYTES; ++k) v[k] = 0;
    });
    return BZK_OK;
}

}  // namespace bzk

using namespace bzk;

extern "C" {

int32_t bzk_ed25519_sign_batch_dev(bzk_ctx* ctx, const void* keys_dev, const void* msg_dev, const void* off_dev, uint64_t n, void* sig_out_dev) {
    if (!ctx || (n && (!keys_dev || !msg_dev || !off_dev || !sig_out_dev))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    const uint64_t rows = n < ED_SIGN_LAUNCH_MAX ? n : ED_SIGN_LAUNCH_MAX;
    WsLayout ws("bzk_ed25519_sign_batch_dev");
    uint8_t* dexp;
    ws.take(dexp, rows * 64);
    BZK_TRY(ws.commit(ctx));
    BZK_TRY(ed25519_sign_launch(ctx, keys_dev, msg_dev, off_dev, (const uint64_t*)off_dev + 1, nullptr, 0, -1, n, dexp, sig_out_dev, nullptr));
    BZK_HIP(ctx, hipMemsetAsync(dexp, 0, rows * 64, ctx->stream));  // the library's own copy of a | prefix goes; the caller's buffers are the caller's
    return BZK_OK;
}

int32_t bzk_ed25519_sign_batch(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* msg, const uint64_t* off, uint64_t n, uint8_t* sig_out) {
    if (n && (!keys || !off || !sig_out)) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (!offsets_ok(off, n) || (off[n] && !msg)) return BZK_E_ARG;
    const uint8_t none = 0;
    if (!msg) msg = &none;  // n empty messages
    if (!ctx) {  // the same per-lane code on host threads
        host_for_each(n, host_default_threads(),
                      [&](uint64_t i) { sign_row_host(keys + 64 * i, sha512::msg_one(msg + off[i], off[i + 1] - off[i]), sig_out + 64 * i); });
        return BZK_OK;
    }
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_ed25519_sign_batch", n, ED25519_SIGN_ROUND, ED25519_SIGN_ROUND_BYTES,
                        lengths(off), off);
    uint8_t *ddata, *doff, *dkeys, *dexp, *dsig;
    st.bytes(ddata, msg, 0, 8); st.offsets(doff); st.in(dkeys, keys, 64); st.scratch(dexp, 64); st.out(dsig, sig_out, 64);
    st.wipe(dkeys, st.cap * 64); st.wipe(dexp, st.cap * 64);  // neither the staged keys nor their expansions outlive the call
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t a, uint64_t m) {
        return ed25519_sign_launch(ctx, dkeys, ddata, doff, doff + 8, nullptr, off[a], -1, m, dexp, dsig, nullptr);
    });
}

int32_t bzk_ed25519_keys_batch_dev(bzk_ctx* ctx, const void* seeds_dev, const void* off_dev, uint64_t n, void* keys_out_dev) {
    if (!ctx || (n && (!seeds_dev || !off_dev || !keys_out_dev))) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    return ed25519_keys_launch(ctx, seeds_dev, off_dev, (const uint64_t*)off_dev + 1, 0, n, keys_out_dev);
}

int32_t bzk_ed25519_keys_batch(bzk_ctx* ctx, const uint8_t* seeds, const uint64_t* off, uint64_t n, uint8_t* keys_out) {
    if (n && (!off || !keys_out)) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (!offsets_ok(off, n) || (off[n] && !seeds)) return BZK_E_ARG;
    const uint8_t none = 0;
    if (!seeds) seeds = &none;  // n empty seeds
    if (!ctx) {  // the same per-lane code on host threads
        const uint32_t* tab = ed25519::base_table_host();
        host_for_each(n, host_default_threads(), [&](uint64_t i) { ed25519::keys_one(seeds + off[i], off[i + 1] - off[i], tab, keys_out + 64 * i); });
        return BZK_OK;
    }
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "bzk_ed25519_keys_batch", n, ED25519_SIGN_ROUND, ED25519_SIGN_ROUND_BYTES,
                        lengths(off), off);
    uint8_t *ddata, *doff, *dkeys;
    st.bytes(ddata, seeds, 0, 8); st.offsets(doff); st.out(dkeys, keys_out, 64);
    st.wipe(ddata, st.cap_bytes + 8); st.wipe(dkeys, st.cap * 64);  // neither the staged seeds nor the keys outlive the call
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t a, uint64_t m) { return ed25519_keys_launch(ctx, ddata, doff, doff + 8, off[a], m, dkeys); });
}

int32_t bzk_host_ed25519_keys(const uint8_t* seed, uint64_t len, uint8_t keys_out[64]) {
    if ((len && !seed) || !keys_out) return BZK_E_ARG;
    const uint8_t none = 0;
    ed25519::keys_one(seed ? seed : &none, len, ed25519::base_table_host(), keys_out);
    return BZK_OK;
}

int32_t bzk_host_ed25519_sign(const uint8_t keys[64], const uint8_t* msg, uint64_t len, uint8_t sig_out[64]) {
    if (!keys || (len && !msg) || !sig_out) return BZK_E_ARG;
    const uint8_t none = 0;
    sign_row_host(keys, sha512::msg_one(msg ? msg : &none, len), sig_out);
    return BZK_OK;
}

}  // extern "C"
