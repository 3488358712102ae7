// Batched subgroup checks (bzk_g1_subgroup_check_batch[_dev], bzk_g2_subgroup_check_batch[_dev]): the third check of bls12_381's
// `from_uncompressed` - canonical, on the curve, of order r - for n raw Montgomery points, one lane per point.  The arithmetic is
// bzk_subgroup.cuh's g1_verdict / g2_verdict; this file holds the two kernels, the rounds and the entry points (the host field's policy for the
// ctx = NULL path: bzk_subgroup_host.h).  No lane waits for another (no LDS, no barrier).  A flagged or invalid record ends its lane before the ladders (the
// only divergence: those lanes leave, the others run on); every lane that enters a ladder runs the same steps whatever its point.
#include "bzk_internal.h"
#include "bzk_stage.h"
#include "bzk_subgroup_host.h"
#include "host_threads.h"

namespace bzk {
namespace {

constexpr int SG_BLOCK = 64;
static_assert(SG_BLOCK == 64, "one wavefront per block: sg_g2_kernel addresses a lane's record and verdict by sg::lane_now(), which is threadIdx.x only then");
constexpr uint64_t SG_ROUND = (uint64_t)1 << 18;  // points per launch; a host-pointer call stages one round of records at a time

__global__ void __launch_bounds__(SG_BLOCK) sg_g1_kernel(const uint32_t* __restrict__ pts, const uint8_t* __restrict__ inf, uint32_t n,
                                                         uint8_t* __restrict__ ok) {
    const uint32_t i = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (inf && inf[i]) {
        ok[i] = sg::IN_SUBGROUP;
        return;
    }
    ok[i] = sg::g1_verdict<sg::SgFp28>(pts + (size_t)24 * i);
}
__global__ void __launch_bounds__(SG_BLOCK) sg_g2_kernel(const uint32_t* __restrict__ pts, const uint8_t* __restrict__ inf, uint32_t n,
                                                         uint8_t* __restrict__ ok) {
    const uint32_t i = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (inf && inf[i]) {
        ok[i] = sg::IN_SUBGROUP;
        return;
    }
    // one wave per block: the block's first record is a uniform address, and the lane index is taken again where the verdict is stored (bzk_subgroup.cuh lane_now)
    const uint8_t v = sg::g2_verdict<sg::SgFp28>(pts + (size_t)48 * SG_BLOCK * blockIdx.x);
    ok[(size_t)blockIdx.x * SG_BLOCK + sg::lane_now()] = v;
}

void host_run(bool g2, const uint8_t* pts, const uint8_t* inf, uint64_t n, uint8_t* ok) {
    const size_t sz = g2 ? 192 : 96;
    host_for_each(n, host_default_threads(), [&](uint64_t i) {
        if (inf && inf[i]) {
            ok[i] = sg::IN_SUBGROUP;
            return;
        }
        uint32_t w[48];
        memcpy(w, pts + sz * i, sz);
        ok[i] = g2 ? sg::g2_verdict<SgHFp>(w) : sg::g1_verdict<SgHFp>(w);
    });
}

// rounds of at most SG_ROUND points whose records, flags and verdict bytes are device pointers
int32_t launch_rounds(bzk_ctx* ctx, bool g2, const uint8_t* pts, const uint8_t* inf, uint64_t n, uint8_t* ok) {
    const size_t sz = g2 ? 192 : 96;
    return launch_rows(n, SG_ROUND, SG_BLOCK, [&](uint64_t a, uint64_t rows, unsigned grid) {
        const uint32_t m = (uint32_t)rows;
        const uint32_t* rp = (const uint32_t*)(pts + sz * a);
        const uint8_t* ri = inf ? inf + a : nullptr;
        if (g2) BZK_LAUNCH(ctx, "sg_g2", sg_g2_kernel, dim3(grid), dim3(SG_BLOCK), 0, rp, ri, m, ok + a);
        else BZK_LAUNCH(ctx, "sg_g1", sg_g1_kernel, dim3(grid), dim3(SG_BLOCK), 0, rp, ri, m, ok + a);
        return BZK_OK;
    });
}

// n records in rounds, the verdicts into host memory.  Host records (on_device false) are staged one round at a time; records that already are in
// device memory (a loaded CRS array) are read where they lie.  The workspace is bounded by the round: records, flags and verdict bytes of SG_ROUND
// points, each round's verdicts copied back behind its kernel
int32_t run_rounds(bzk_ctx* ctx, const char* who, bool g2, const uint8_t* pts, bool on_device, const uint8_t* inf, uint64_t n, uint8_t* ok) {
    (void)hipSetDevice(ctx->device);
    const size_t sz = g2 ? 192 : 96;
    Stage<StreamOps> st({ctx}, who, n, SG_ROUND);
    uint8_t *dp = nullptr, *di = nullptr, *dok = nullptr;
    if (!on_device) {
        st.in(dp, pts, sz);
        if (inf) st.in(di, inf, 1);
    }
    st.out(dok, ok, 1);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t a, uint64_t m) {
        if (on_device) return launch_rounds(ctx, g2, pts + sz * a, inf ? inf + a : nullptr, m, dok);
        return launch_rounds(ctx, g2, dp, di, m, dok);
    });
}

int32_t entry_host_ptrs(bzk_ctx* ctx, const char* who, bool g2, const uint8_t* pts, const uint8_t* inf, uint64_t n, uint8_t* ok) {
    if (n == 0) return BZK_OK;
    if (!pts || !ok) return BZK_E_ARG;
    if (!ctx) {
        host_run(g2, pts, inf, n, ok);
        return BZK_OK;
    }
    return run_rounds(ctx, who, g2, pts, false, inf, n, ok);
}
int32_t entry_dev_ptrs(bzk_ctx* ctx, bool g2, const void* pts, const void* inf, uint64_t n, void* ok) {
    if (!ctx) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (!pts || !ok || ((uintptr_t)pts & 3)) return BZK_E_ARG;  // the records are read as 32-bit words
    (void)hipSetDevice(ctx->device);
    BZK_TRY(launch_rounds(ctx, g2, (const uint8_t*)pts, (const uint8_t*)inf, n, (uint8_t*)ok));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BZK_OK;
}

}  // namespace

// ---- for the checked parameter reader (host_bellman.hip): *idx = the first of n finite records whose verdict is not 1 (n: none), *code = its verdict.
// ctx = NULL: host threads on host records; on_device: the records are in device memory already
int32_t sg_first_bad(bzk_ctx* ctx, const char* who, bool g2, const uint8_t* pts, bool on_device, uint64_t n, uint64_t* idx, uint8_t* code) {
    *idx = n;
    *code = sg::IN_SUBGROUP;
    if (n == 0) return BZK_OK;
    std::vector<uint8_t> ok(n);
    if (!ctx) host_run(g2, pts, nullptr, n, ok.data());
    else BZK_TRY(run_rounds(ctx, who, g2, pts, on_device, nullptr, n, ok.data()));
    for (uint64_t i = 0; i < n; ++i)
        if (ok[i] != sg::IN_SUBGROUP) {
            *idx = i;
            *code = ok[i];
            break;
        }
    return BZK_OK;
}
uint8_t sg_host_one(bool g2, const uint8_t* raw) {
    uint8_t v = 0;
    host_run(g2, raw, nullptr, 1, &v);
    return v;
}

}  // namespace bzk

using namespace bzk;

extern "C" {

int32_t bzk_g1_subgroup_check_batch(bzk_ctx* ctx, const uint8_t* pts, const uint8_t* inf, uint64_t n, uint8_t* ok) {
    return entry_host_ptrs(ctx, "bzk_g1_subgroup_check_batch", false, pts, inf, n, ok);
}
int32_t bzk_g1_subgroup_check_batch_dev(bzk_ctx* ctx, const void* pts_dev, const void* inf_dev, uint64_t n, void* ok_dev) {
    return entry_dev_ptrs(ctx, false, pts_dev, inf_dev, n, ok_dev);
}
int32_t bzk_g2_subgroup_check_batch(bzk_ctx* ctx, const uint8_t* pts, const uint8_t* inf, uint64_t n, uint8_t* ok) {
    return entry_host_ptrs(ctx, "bzk_g2_subgroup_check_batch", true, pts, inf, n, ok);
}
int32_t bzk_g2_subgroup_check_batch_dev(bzk_ctx* ctx, const void* pts_dev, const void* inf_dev, uint64_t n, void* ok_dev) {
    return entry_dev_ptrs(ctx, true, pts_dev, inf_dev, n, ok_dev);
}

}  // extern "C"
