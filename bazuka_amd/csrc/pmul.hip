// n points times n scalars on G1 and G2 (bzk_g1_mul_batch[_dev], bzk_g2_mul_batch[_dev]) and the powers form out[i] = c s^(start + i) pts[i]
// (bzk_g1_mul_powers[_dev], bzk_g2_mul_powers[_dev]).  The per-point arithmetic and the row of a recoded scalar are bzk_pmul.cuh's mul_point and
// row_of; this file holds the kernels, the rounds and the entry points.  A call is two launches per round: the preparation (scalar -> nine words,
// cheap) and the multiplication (a fixed 128 steps per lane).  No lane waits for another (no LDS, no barrier); no step of a lane depends on its point.
#include <string.h>

#include <atomic>

#include "bzk_internal.h"
#include "bzk_pmul.cuh"
#include "bzk_pmul.h"
#include "bzk_stage.h"
#include "bzk_subgroup_host.h"
#include "host_threads.h"

namespace bzk {
namespace {

constexpr int PM_BLOCK = 64;
static_assert(PM_BLOCK == 64, "one wavefront per block: g2_pmul_kernel addresses a lane's record by sg::lane_now(), which is threadIdx.x only then");
constexpr uint64_t PM_ROUND = (uint64_t)1 << 18;      // points per staged round of a host-pointer call (rekey.hip's)
constexpr uint64_t PM_DEV_ROUND = (uint64_t)1 << 22;  // points per launch over device-resident records: the rows of one round are 144 MiB
constexpr int TAB = 65;                               // c, then s^(2^j) for j < 64

// *bad = 1 when one of n scalars has limbs that are not below r (Montgomery or canonical: the same test)
__global__ void __launch_bounds__(PM_BLOCK) pmul_range_kernel(const uint32_t* __restrict__ sc, uint32_t n, uint32_t* __restrict__ bad) {
    const uint32_t i = blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= n) return;
    Fr k;
#pragma unroll
    for (int j = 0; j < 8; ++j) k.l[j] = sc[(size_t)8 * i + j];
    if (!pm::below_r(k)) *bad = 1;
}

__global__ void __launch_bounds__(PM_BLOCK) pmul_prep_kernel(const uint32_t* __restrict__ sc, uint32_t n, uint32_t canonical, uint32_t* __restrict__ rows) {
    const uint32_t i = blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= n) return;
    Fr k;
#pragma unroll
    for (int j = 0; j < 8; ++j) k.l[j] = sc[(size_t)8 * i + j];
    if (!canonical) k = fe_from_mont<FrParams>(k);
    uint32_t row[pm::ROW_WORDS];
    pm::row_of(k.l, row);
#pragma unroll
    for (int j = 0; j < pm::ROW_WORDS; ++j) rows[(size_t)pm::ROW_WORDS * i + j] = row[j];
}

// row i of the round: c s^(first + i), from the table tab = c | s^(2^j)
__global__ void __launch_bounds__(PM_BLOCK) pmul_prep_powers_kernel(const Fr* __restrict__ tab, uint64_t first, uint32_t n, uint32_t* __restrict__ rows) {
    const uint32_t i = blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const Fr k = fe_from_mont<FrParams>(pm::power_of(tab[0], tab + 1, first + i));
    uint32_t row[pm::ROW_WORDS];
    pm::row_of(k.l, row);
#pragma unroll
    for (int j = 0; j < pm::ROW_WORDS; ++j) rows[(size_t)pm::ROW_WORDS * i + j] = row[j];
}

// out may be pts (a lane has read its record for the last time before it writes): neither is __restrict__
__global__ void __launch_bounds__(PM_BLOCK) g1_pmul_kernel(const uint32_t* pts, uint32_t n, const uint32_t* rows, uint32_t* out, uint8_t* inf) {
    const uint32_t i = blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t v = pm::mul_point<pm::PmG1<sc::ScFp28>>(pts + (size_t)24 * i, rows + (size_t)pm::ROW_WORDS * i, out + (size_t)24 * i);
    if (inf) inf[i] = v;
}
// one wave per block: the block's first record is a uniform address, and the lane index is taken again where the result is stored
__global__ void __launch_bounds__(PM_BLOCK) g2_pmul_kernel(const uint32_t* pts, uint32_t n, const uint32_t* rows, uint32_t* out, uint8_t* inf) {
    const uint32_t i = blockIdx.x * PM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t first = (size_t)PM_BLOCK * blockIdx.x;
    const uint8_t v = pm::mul_point<pm::PmG2<sc::ScFp28>>(pts + 48 * first, rows + (size_t)pm::ROW_WORDS * i, out + 48 * first);
    if (inf) inf[first + sg::lane_now()] = v;
}

Fr fr_load(const uint8_t* p) {
    Fr a;
    memcpy(a.l, p, 32);
    return a;
}
// c | s^(2^j), j < 64
void power_table(const Fr& c, const Fr& s, Fr tab[TAB]) {
    tab[0] = c;
    tab[1] = s;
    for (int j = 2; j < TAB; ++j) tab[j] = fe_sqr<FrParams>(tab[j - 1]);
}

void host_run(const PmCall& k, const Fr* tab) {
    const size_t sz = k.g2 ? 192 : 96;
    host_for_each(k.n, host_default_threads(), [&](uint64_t i) {
        Fr kc = tab ? pm::power_of(tab[0], tab + 1, k.start + i) : fr_load(k.scalars + 32 * i);
        if (tab || !k.canonical) kc = fe_from_mont<FrParams>(kc);
        uint32_t row[pm::ROW_WORDS], w[48], o[48];
        pm::row_of(kc.l, row);
        memcpy(w, k.pts + sz * i, sz);
        const uint8_t v = k.g2 ? pm::mul_point<pm::PmG2<SgHFp>>(w, row, o) : pm::mul_point<pm::PmG1<SgHFp>>(w, row, o);
        memcpy(k.out + sz * i, o, sz);
        if (k.inf) k.inf[i] = v;
        wipe_host(&kc, sizeof kc);
        wipe_host(row, sizeof row);
    });
}

// the rounds of one call.  Host records and scalars go up and the results come back through one staging buffer per round (the kernel runs in
// place); records in device memory are read and written where they lie.  The rows and the table are buffers of the call's layout on the wipe list
int32_t run_rounds(bzk_ctx* ctx, const char* who, const PmCall& k, const Fr* tab) {
    (void)hipSetDevice(ctx->device);
    const size_t sz = k.g2 ? 192 : 96;
    Stage<StreamOps> st({ctx}, who, k.n, k.on_device ? PM_DEV_ROUND : PM_ROUND);
    uint8_t *dp = nullptr, *di = nullptr, *dsc = nullptr, *drows = nullptr, *dtab = nullptr, *dbad = nullptr;
    if (!k.on_device) {
        st.in(dp, k.pts, sz);
        st.out_part(dp, k.out, sz, 0);
        st.out(di, k.inf, 1);
        if (!tab) st.in(dsc, k.scalars, 32);
    }
    st.scratch(drows, 4 * pm::ROW_WORDS);
    st.wipe(drows, st.cap * 4 * pm::ROW_WORDS);
    if (tab) {
        st.ws.take(dtab, TAB * sizeof(Fr));
        st.wipe(dtab, TAB * sizeof(Fr));
    } else if (k.on_device) {
        st.ws.take(dbad, 4);
    }
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t a, uint64_t m) {
        if (a == 0 && tab) BZK_TRY(st.dev.up(dtab, tab, TAB * sizeof(Fr)));
        if (a == 0 && dbad) {  // scalars in device memory: all of them are tested before the first record is written
            uint32_t bad = 0;
            BZK_TRY(st.dev.zero(dbad, 4));
            for (uint64_t at = 0; at < k.n; at += PM_DEV_ROUND) {
                const uint64_t cnt = k.n - at < PM_DEV_ROUND ? k.n - at : PM_DEV_ROUND;
                BZK_LAUNCH(ctx, "pmul_range", pmul_range_kernel, dim3((unsigned)((cnt + PM_BLOCK - 1) / PM_BLOCK)), dim3(PM_BLOCK), 0,
                           (const uint32_t*)(k.scalars + 32 * at), (uint32_t)cnt, (uint32_t*)dbad);
            }
            BZK_TRY(st.dev.down(&bad, dbad, 4));
            BZK_TRY(st.dev.sync());
            if (bad) return (int32_t)BZK_E_ARG;
        }
        const dim3 grid((unsigned)((m + PM_BLOCK - 1) / PM_BLOCK)), block(PM_BLOCK);
        if (tab)
            BZK_LAUNCH(ctx, "pmul_prep_powers", pmul_prep_powers_kernel, grid, block, 0, (const Fr*)dtab, k.start + a, (uint32_t)m, (uint32_t*)drows);
        else
            BZK_LAUNCH(ctx, "pmul_prep", pmul_prep_kernel, grid, block, 0, (const uint32_t*)(k.on_device ? k.scalars + 32 * a : dsc), (uint32_t)m,
                       k.canonical ? 1u : 0u, (uint32_t*)drows);
        const uint32_t* src = (const uint32_t*)(k.on_device ? k.pts + sz * a : dp);
        uint32_t* dst = (uint32_t*)(k.on_device ? k.out + sz * a : dp);
        uint8_t* flags = k.on_device ? (k.inf ? k.inf + a : nullptr) : di;
        if (k.g2) BZK_LAUNCH(ctx, "g2_pmul", g2_pmul_kernel, grid, block, 0, src, (uint32_t)m, (const uint32_t*)drows, dst, flags);
        else BZK_LAUNCH(ctx, "g1_pmul", g1_pmul_kernel, grid, block, 0, src, (uint32_t)m, (const uint32_t*)drows, dst, flags);
        return (int32_t)BZK_OK;
    });
}

}  // namespace

int32_t pm_run(bzk_ctx* ctx, const char* who, const PmCall& k) {
    Fr tab[TAB];
    const bool powers = k.scalars == nullptr;
    if (powers) {
        Fr c = fr_load(k.c), s = fr_load(k.s);
        const bool ok = pm::below_r(c) && pm::below_r(s) && k.start + k.n >= k.start;
        if (ok && k.n) power_table(c, s, tab);
        wipe_host(&c, sizeof c);
        wipe_host(&s, sizeof s);
        if (!ok) return BZK_E_ARG;
    } else if (!k.on_device) {  // host scalars: all of them are tested before the first record is written
        std::atomic<uint32_t> bad(0);
        const uint64_t chunk = 4096;
        host_for_each((k.n + chunk - 1) / chunk, host_default_threads(), [&](uint64_t c) {
            for (uint64_t i = c * chunk; i < k.n && i < (c + 1) * chunk; ++i)
                if (!pm::below_r(fr_load(k.scalars + 32 * i))) bad.store(1);
        });
        if (bad.load()) return BZK_E_ARG;
    }
    if (k.n == 0) return BZK_OK;
    int32_t st = BZK_OK;
    if (!ctx) host_run(k, powers ? tab : nullptr);
    else st = run_rounds(ctx, who, k, powers ? tab : nullptr);
    wipe_host(tab, sizeof tab);
    return st;
}

}  // namespace bzk

using namespace bzk;

namespace {

int32_t batch_entry(bzk_ctx* ctx, const char* who, bool g2, bool dev, const void* pts, const void* scalars, uint64_t n, uint32_t flags, void* out,
                    void* inf) {
    if (dev && !ctx) return BZK_E_ARG;
    if (n && (!pts || !scalars || !out)) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    if (dev && (((uintptr_t)pts | (uintptr_t)scalars | (uintptr_t)out) & 3)) return BZK_E_ARG;  // read and written as 32-bit words
    PmCall k;
    k.g2 = g2;
    k.pts = (const uint8_t*)pts;
    k.on_device = dev;
    k.n = n;
    k.scalars = (const uint8_t*)scalars;
    k.canonical = (flags & BZK_F_CANONICAL) != 0;
    k.out = (uint8_t*)out;
    k.inf = (uint8_t*)inf;
    return pm_run(ctx, who, k);
}
int32_t powers_entry(bzk_ctx* ctx, const char* who, bool g2, bool dev, const void* pts, uint64_t n, const uint8_t* c, const uint8_t* s, uint64_t start,
                     void* out, void* inf) {
    if (dev && !ctx) return BZK_E_ARG;
    if (!c || !s || (n && (!pts || !out))) return BZK_E_ARG;
    if (dev && (((uintptr_t)pts | (uintptr_t)out) & 3)) return BZK_E_ARG;
    PmCall k;
    k.g2 = g2;
    k.pts = (const uint8_t*)pts;
    k.on_device = dev;
    k.n = n;
    k.c = c;
    k.s = s;
    k.start = start;
    k.out = (uint8_t*)out;
    k.inf = (uint8_t*)inf;
    return pm_run(ctx, who, k);
}

}  // namespace

extern "C" {

int32_t bzk_g1_mul_batch(bzk_ctx* ctx, const uint8_t* pts, const uint8_t* scalars, uint64_t n, uint32_t flags, uint8_t* out, uint8_t* inf_out) {
    return batch_entry(ctx, "bzk_g1_mul_batch", false, false, pts, scalars, n, flags, out, inf_out);
}
int32_t bzk_g1_mul_batch_dev(bzk_ctx* ctx, const void* pts_dev, const void* scalars_dev, uint64_t n, uint32_t flags, void* out_dev, void* inf_out_dev) {
    return batch_entry(ctx, "bzk_g1_mul_batch_dev", false, true, pts_dev, scalars_dev, n, flags, out_dev, inf_out_dev);
}
int32_t bzk_g2_mul_batch(bzk_ctx* ctx, const uint8_t* pts, const uint8_t* scalars, uint64_t n, uint32_t flags, uint8_t* out, uint8_t* inf_out) {
    return batch_entry(ctx, "bzk_g2_mul_batch", true, false, pts, scalars, n, flags, out, inf_out);
}
int32_t bzk_g2_mul_batch_dev(bzk_ctx* ctx, const void* pts_dev, const void* scalars_dev, uint64_t n, uint32_t flags, void* out_dev, void* inf_out_dev) {
    return batch_entry(ctx, "bzk_g2_mul_batch_dev", true, true, pts_dev, scalars_dev, n, flags, out_dev, inf_out_dev);
}
int32_t bzk_g1_mul_powers(bzk_ctx* ctx, const uint8_t* pts, uint64_t n, const uint8_t c[32], const uint8_t s[32], uint64_t start, uint8_t* out,
                          uint8_t* inf_out) {
    return powers_entry(ctx, "bzk_g1_mul_powers", false, false, pts, n, c, s, start, out, inf_out);
}
int32_t bzk_g1_mul_powers_dev(bzk_ctx* ctx, const void* pts_dev, uint64_t n, const uint8_t c[32], const uint8_t s[32], uint64_t start, void* out_dev,
                              void* inf_out_dev) {
    return powers_entry(ctx, "bzk_g1_mul_powers_dev", false, true, pts_dev, n, c, s, start, out_dev, inf_out_dev);
}
int32_t bzk_g2_mul_powers(bzk_ctx* ctx, const uint8_t* pts, uint64_t n, const uint8_t c[32], const uint8_t s[32], uint64_t start, uint8_t* out,
                          uint8_t* inf_out) {
    return powers_entry(ctx, "bzk_g2_mul_powers", true, false, pts, n, c, s, start, out, inf_out);
}
int32_t bzk_g2_mul_powers_dev(bzk_ctx* ctx, const void* pts_dev, uint64_t n, const uint8_t c[32], const uint8_t s[32], uint64_t start, void* out_dev,
                              void* inf_out_dev) {
    return powers_entry(ctx, "bzk_g2_mul_powers_dev", true, true, pts_dev, n, c, s, start, out_dev, inf_out_dev);
}

}  // extern "C"
