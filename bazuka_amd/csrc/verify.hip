// Batched Groth16 verification (bzk_groth16_verify_batch[_dev]): `groth16_verify` (src/zk/groth16/mod.rs:67-121) for n proofs of ONE verifying key,
// one lane per proof.  The arithmetic is bzk_pairing28.cuh's prepare_one / miller_one / finalexp_one; this file holds what is done once per call
// on the host (the key's window tables, the line coefficients of its fixed G2 arguments, its constant Miller value), the three kernels and the
// two entry points.  A proof's state lives in its column of a limb-major slab of the call's workspace (pairing::slot), never in private arrays:
// the kernels differ only in which step they run, so each stays one instruction cache long, has its own launch bounds, and a fault names its stage.
// No lane waits for another (no LDS, no barrier): a lane that has its verdict simply returns.
#include "bzk_internal.h"
#include "host_pairing.h"
#include "host_threads.h"

namespace bzk {
namespace {

using pairing::KeyView;
using pairing::Lane28;
typedef KeyView<Fp28Ops, Fp2x28Ops> KeyDev;
typedef KeyView<HFpOps, HFp2Ops> KeyHostView;
using hp::KeyHost;
using hp::KeyUpload;
using hp::key_prepare;

constexpr int G16V_BLOCK = 64;
constexpr uint64_t G16V_ROUND = (uint64_t)1 << 16;   // proofs per round of launches; a later round reuses the slab
constexpr uint32_t G16V_MAX_INPUTS = 16;             // above: the host-thread path.  A limit of the interface, not of the workspace (sized by n_inputs)

__global__ void __launch_bounds__(G16V_BLOCK) g16v_prepare_kernel(KeyDev k, const uint8_t* __restrict__ inputs, const uint8_t* __restrict__ proofs,
                                                                  uint32_t n, uint32_t* __restrict__ slab, uint32_t stride,
                                                                  uint32_t* __restrict__ sc, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * G16V_BLOCK + threadIdx.x;
    if (i >= n) return;
    // sc: word j of lane i at sc[j * stride + i], word-major as the slab
    flags[i] = pairing::prepare_one(Lane28{slab + i, stride}, k, inputs + (size_t)32 * k.n_inputs * i, proofs + (size_t)387 * i, sc + i, stride);
}
__global__ void __launch_bounds__(G16V_BLOCK) g16v_miller_kernel(KeyDev k, uint32_t n, uint32_t* __restrict__ slab, uint32_t stride,
                                                                 uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * G16V_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flags[i];
    if (f & pairing::FLAG_REFUSED) return;
    flags[i] = pairing::miller_one(Lane28{slab + i, stride}, k, f);
}
__global__ void __launch_bounds__(G16V_BLOCK) g16v_finalexp_kernel(KeyDev k, uint32_t n, uint32_t* __restrict__ slab, uint32_t stride,
                                                                   const uint32_t* __restrict__ flags, uint8_t* __restrict__ ok) {
    const uint32_t i = blockIdx.x * G16V_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (flags[i] & (pairing::FLAG_REFUSED | pairing::FLAG_DEGENERATE)) {
        ok[i] = 0;
        return;
    }
    ok[i] = pairing::finalexp_one(Lane28{slab + i, stride}, k) ? 1 : 0;
}

// the per-lane functions over the host field, one proof per task
void host_run(const KeyHost& K, const uint8_t* inputs, const uint8_t* proofs, uint64_t n, uint8_t* ok) {
    if (!K.valid) {
        memset(ok, 0, n);
        return;
    }
    const KeyHostView k = K.view();
    host_for_each(n, host_default_threads(), [&](uint64_t i) {
        HFp slab[pairing::slot::COUNT];
        thread_local std::vector<uint32_t> sc;   // the canonical scalars: sized once per thread, not per proof
        if (sc.size() < (size_t)8 * K.n_inputs + 1) sc.resize((size_t)8 * K.n_inputs + 1);
        const hp::LaneH l = {slab};
        uint32_t f = pairing::prepare_one(l, k, inputs + (size_t)32 * K.n_inputs * i, proofs + 387 * i, sc.data(), 1);
        if (!(f & pairing::FLAG_REFUSED)) f = pairing::miller_one(l, k, f);
        ok[i] = (f & (pairing::FLAG_REFUSED | pairing::FLAG_DEGENERATE)) ? 0 : (pairing::finalexp_one(l, k) ? 1 : 0);
    });
}

// one round of launches over m <= G16V_ROUND proofs whose inputs, proofs and verdict bytes are device pointers
int32_t launch_round(bzk_ctx* ctx, const G16vBufs& b, const KeyDev& k, const uint8_t* rin, const uint8_t* rpr, uint32_t m, uint8_t* rok) {
    const dim3 grid((m + G16V_BLOCK - 1) / G16V_BLOCK), block(G16V_BLOCK);
    BZK_LAUNCH(ctx, "g16v_prepare", g16v_prepare_kernel, grid, block, 0, k, rin, rpr, m, b.slab, b.stride, b.sc, b.flags);
    BZK_LAUNCH(ctx, "g16v_miller", g16v_miller_kernel, grid, block, 0, k, m, b.slab, b.stride, b.flags);
    BZK_LAUNCH(ctx, "g16v_finalexp", g16v_finalexp_kernel, grid, block, 0, k, m, b.slab, b.stride, (const uint32_t*)b.flags, rok);
    return BZK_OK;
}

// inputs / proofs / ok: host pointers (staged per round, verdicts read back once) when `staged`, device pointers otherwise
int32_t device_run(bzk_ctx* ctx, const char* who, const KeyHost& K, const uint8_t* inputs, const uint8_t* proofs, uint64_t n, uint8_t* ok, bool staged) {
    (void)hipSetDevice(ctx->device);
    if (!K.valid) {
        if (staged) memset(ok, 0, n);
        else {
            BZK_HIP(ctx, hipMemsetAsync(ok, 0, n, ctx->stream));
            BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        return BZK_OK;
    }
    const KeyUpload up(K);   // the tables in the device field
    const uint64_t cap = std::min<uint64_t>(n, G16V_ROUND);
    const size_t in_bytes = (size_t)32 * K.n_inputs;
    WsLayout ws(who);
    G16vBufs b;
    uint8_t *din = nullptr, *dpr = nullptr, *dok = nullptr;
    g16v_declare(ws, b, K.n_inputs, n, up.bytes.size());
    if (staged) {
        ws.take(din, in_bytes * cap + 1);
        ws.take(dpr, (size_t)387 * cap);
        ws.take(dok, n);
    }
    BZK_TRY(ws.commit(ctx));
    if (!staged) return g16v_enqueue(ctx, b, K, up, inputs, proofs, n, ok, true);
    BZK_HIP(ctx, hipMemcpyAsync(b.dkey, up.bytes.data(), up.bytes.size(), hipMemcpyHostToDevice, ctx->stream));
    const KeyDev k = up.view(K, b.dkey);
    for (uint64_t a = 0; a < n; a += G16V_ROUND) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(n - a, G16V_ROUND);
        if (in_bytes) BZK_HIP(ctx, hipMemcpyAsync(din, inputs + in_bytes * a, in_bytes * m, hipMemcpyHostToDevice, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(dpr, proofs + 387 * a, (size_t)387 * m, hipMemcpyHostToDevice, ctx->stream));
        BZK_TRY(launch_round(ctx, b, k, din, dpr, m, dok + a));
    }
    BZK_HIP(ctx, hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the key's upload buffer and the layout go out of scope here
    return BZK_OK;
}

}  // namespace

// ---- the verifier as a stage of another call (updates.hip): that call declares these buffers in ITS layout, commits once, and enqueues here.
// A context takes one committed layout at a time (the slab moves when it grows), so a call cannot nest bzk_groth16_verify_batch_dev in its own.
void g16v_declare(WsLayout& ws, G16vBufs& b, uint32_t n_inputs, uint64_t n, size_t key_bytes) {
    const uint64_t cap = std::min<uint64_t>(n, G16V_ROUND);
    b.stride = (uint32_t)((cap + G16V_BLOCK - 1) / G16V_BLOCK * G16V_BLOCK);
    ws.take(b.slab, (size_t)pairing::slot::COUNT * 14 * b.stride);
    ws.take(b.flags, b.stride);
    ws.take(b.sc, (size_t)8 * n_inputs * b.stride + 1);
    ws.take(b.dkey, key_bytes);
}
// n proofs of the valid key K on a committed layout: the key's tables go up, then rounds of G16V_ROUND proofs.  Device pointers; `up` must outlive
// the stream's work.  sync: wait for it here
int32_t g16v_enqueue(bzk_ctx* ctx, const G16vBufs& b, const KeyHost& K, const KeyUpload& up, const uint8_t* inputs_dev, const uint8_t* proofs_dev,
                     uint64_t n, uint8_t* ok_dev, bool sync) {
    BZK_HIP(ctx, hipMemcpyAsync(b.dkey, up.bytes.data(), up.bytes.size(), hipMemcpyHostToDevice, ctx->stream));
    const KeyDev k = up.view(K, b.dkey);
    const size_t in_bytes = (size_t)32 * K.n_inputs;
    for (uint64_t a = 0; a < n; a += G16V_ROUND) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(n - a, G16V_ROUND);
        BZK_TRY(launch_round(ctx, b, k, inputs_dev + in_bytes * a, proofs_dev + 387 * a, m, ok_dev + a));
    }
    if (sync) BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BZK_OK;
}
void g16v_host_run(const KeyHost& K, const uint8_t* inputs, const uint8_t* proofs, uint64_t n, uint8_t* ok) { host_run(K, inputs, proofs, n, ok); }

}  // namespace bzk

using namespace bzk;

extern "C" {

int32_t bzk_groth16_verify_batch(bzk_ctx* ctx, const uint8_t* vk, uint64_t vk_len, const uint8_t* inputs, uint32_t n_inputs, const uint8_t* proofs,
                                 uint64_t n, uint8_t* ok) {
    if (n == 0) return BZK_OK;
    if (!vk || !proofs || !ok || (n_inputs && !inputs)) return BZK_E_ARG;
    if (vk_len < 878) return BZK_E_ARG;
    KeyHost K;
    key_prepare(vk, vk_len, n_inputs, K);
    if (!ctx || n_inputs > G16V_MAX_INPUTS) {
        host_run(K, inputs, proofs, n, ok);
        return BZK_OK;
    }
    return device_run(ctx, "bzk_groth16_verify_batch", K, inputs, proofs, n, ok, true);
}

int32_t bzk_groth16_verify_batch_dev(bzk_ctx* ctx, const uint8_t* vk, uint64_t vk_len, const void* inputs_dev, uint32_t n_inputs,
                                     const void* proofs_dev, uint64_t n, void* ok_dev) {
    if (!ctx) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (!vk || !proofs_dev || !ok_dev || (n_inputs && !inputs_dev)) return BZK_E_ARG;
    if (vk_len < 878) return BZK_E_ARG;
    KeyHost K;
    key_prepare(vk, vk_len, n_inputs, K);
    if (n_inputs > G16V_MAX_INPUTS) {   // the host-thread path on copies
        (void)hipSetDevice(ctx->device);
        std::vector<uint8_t> hin((size_t)32 * n_inputs * n), hpr((size_t)387 * n), hok(n);
        BZK_HIP(ctx, hipMemcpyAsync(hin.data(), inputs_dev, hin.size(), hipMemcpyDeviceToHost, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(hpr.data(), proofs_dev, hpr.size(), hipMemcpyDeviceToHost, ctx->stream));
        BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        host_run(K, hin.data(), hpr.data(), n, hok.data());
        BZK_HIP(ctx, hipMemcpyAsync(ok_dev, hok.data(), n, hipMemcpyHostToDevice, ctx->stream));
        BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return BZK_OK;
    }
    return device_run(ctx, "bzk_groth16_verify_batch_dev", K, (const uint8_t*)inputs_dev, (const uint8_t*)proofs_dev, n, (uint8_t*)ok_dev, false);
}

}  // extern "C"
