// Batched Jubjub EdDSA verification on the device (bzk_jubjub_verify_batch[_dev]): `JubJub::<ZkHasher>::verify` (src/crypto/jubjub/mod.rs:151-167) for
// n independent (key, message, signature) triples, one lane per signature.  The arithmetic is bzk_eddsa.cuh's verify_one; this file holds the kernel,
// the per-context table of multiples of BASE and the two entry points.

// The hash is a quarter of a verification and shares its kernel with the ladders: its MDS matrix is re-read in every full round (scalar loads) instead of
// being hoisted out of the round loop into 324 scalars the register file does not have (bzk_poseidon29.cuh)
#define BZK_POSEIDON_MDS_RELOAD 1
#include "bzk_eddsa.cuh"
#include "bzk_internal.h"

namespace bzk {

int32_t poseidon_consts_dev_shared(bzk_ctx* ctx, int t, const void** out, int* rf, int* rp);  // poseidon.hip

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

static int32_t eddsa_table_dev(bzk_ctx* ctx, const Fr29** out) {
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
    for (uint64_t off = 0; off < n; off += EDDSA_LAUNCH_MAX) {
        const uint64_t m = n - off < EDDSA_LAUNCH_MAX ? n - off : EDDSA_LAUNCH_MAX;
        BZK_LAUNCH(ctx, "jubjub_verify", jubjub_verify_kernel, dim3((unsigned)((m + EDDSA_BLOCK - 1) / EDDSA_BLOCK)), dim3(EDDSA_BLOCK), 0,
                   (const Fr*)pub_xy_dev + 2 * off, (const Fr*)msg_dev + off, (const Fr*)sig_dev + 3 * off, m, (const Fr29*)pconsts, rf, rp, tab,
                   (uint8_t*)ok_dev + off);
    }
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
    constexpr uint64_t CHUNK = (uint64_t)1 << 20;  // 193 bytes per signature: at most 193 MB of workspace
    const uint64_t cap = n < CHUNK ? n : CHUNK;
    BZK_TRY(ws_reserve(ctx, ws_pad(cap * 64) + ws_pad(cap * 32) + ws_pad(cap * 96) + ws_pad(cap) + 1024));
    WsCursor cur(ctx->ws);
    uint8_t* dpub = cur.take<uint8_t>(cap * 64);
    uint8_t* dmsg = cur.take<uint8_t>(cap * 32);
    uint8_t* dsig = cur.take<uint8_t>(cap * 96);
    uint8_t* dok = cur.take<uint8_t>(cap);
    for (uint64_t off = 0; off < n; off += CHUNK) {  // one stream: a chunk's uploads follow the previous chunk's kernel
        const uint64_t m = n - off < CHUNK ? n - off : CHUNK;
        BZK_HIP(ctx, hipMemcpyAsync(dpub, pub_xy + off * 64, m * 64, hipMemcpyHostToDevice, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(dmsg, msg + off * 32, m * 32, hipMemcpyHostToDevice, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(dsig, sig + off * 96, m * 96, hipMemcpyHostToDevice, ctx->stream));
        BZK_TRY(jubjub_verify_launch(ctx, dpub, dmsg, dsig, m, dok));
        BZK_HIP(ctx, hipMemcpyAsync(ok + off, dok, m, hipMemcpyDeviceToHost, ctx->stream));
    }
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BZK_OK;
}

}  // extern "C"
