// A.z, B.z, C.z from the witness alone (bzk_r1cs_mats_*, bzk_r1cs_eval*): the three matrices of a circuit shape made resident once, then one launch
// per evaluation.  The arithmetic, the chunk bound and the resident form are bzk_r1cs_eval.cuh's; this file holds the handle, the loader, the two
// kernels and the host-thread route.  bzk_groth16_prove_witness (groth16.hip) enqueues the same launch into a slot's d_a / d_b / d_c.
//
// r1cs_eval_kernel, grid (x, 3): plane y evaluates matrix y.  Blocks [0, short_blocks) give every row of at most SHORT_MAX entries a lane (a wave then
// waits for two chunks at the most) and, behind those rows, write the zeros of rows n_rows .. pad_rows; the blocks after them give every longer row a
// wave - lane l sums the chunks l, l + 64, ... and the 64 partial sums are added through the lanes' registers.  The split is made when the handle
// is built, where every row's length is known.
#include <algorithm>
#include <atomic>
#include <new>
#include <string>
#include <vector>

#include "bzk_internal.h"
#include "bzk_r1cs_eval.cuh"
#include "host_threads.h"

using bzk::Fr;
using bzk::Fr29;
namespace r1e = bzk::r1e;
namespace fr29 = bzk::fr29;

struct bzk_r1cs_mats {
    bzk_ctx* owner = nullptr;  // the context it was loaded with; nullptr: host memory, host-thread route only
    int device = -1;
    uint32_t n_in = 0, n_aux = 0;
    uint64_t n_rows = 0, nnz[3] = {0, 0, 0}, n_dict = 0, n_pm1 = 0, bytes = 0;
    r1e::HostMats host;          // kept for a handle without a context only
    void* dev = nullptr;         // one allocation: the Mat records, then every array
    const r1e::Mat* d_mats = nullptr;
    uint32_t n_short[3] = {0, 0, 0}, long_blocks[3] = {0, 0, 0};  // rows that take a lane each; blocks of the rows that take a wave each
};

namespace bzk {

static constexpr uint32_t EVAL_BLOCK = 256;

__global__ void __launch_bounds__(256) r1cs_eval_kernel(const r1e::Mat* __restrict__ mats, const Fr* __restrict__ z, Fr* __restrict__ out_a,
                                                        Fr* __restrict__ out_b, Fr* __restrict__ out_c, uint64_t pad_rows) {
    const uint32_t k = blockIdx.y;
    Fr* const out = k == 0 ? out_a : (k == 1 ? out_b : out_c);
    if (!out) return;
    const r1e::Mat M = mats[k];
    const uint64_t n_pad = pad_rows - M.n_rows;
    const uint64_t short_blocks = ((uint64_t)M.n_short + n_pad + EVAL_BLOCK - 1) / EVAL_BLOCK;
    if (blockIdx.x < short_blocks) {
        const uint64_t i = (uint64_t)blockIdx.x * EVAL_BLOCK + threadIdx.x;
        if (i < M.n_short) {
            const uint32_t row = M.short_rows[i];
            out[row] = r1e::row_eval(M, z, row);
        } else if (i - M.n_short < n_pad) {
            out[M.n_rows + (i - M.n_short)] = Fr::zero();
        }
        return;
    }
    const uint64_t w = ((uint64_t)blockIdx.x - short_blocks) * (EVAL_BLOCK / r1e::WAVE) + threadIdx.x / r1e::WAVE;
    if (w >= M.n_long) return;  // the whole wave leaves
    const uint32_t row = M.long_rows[w], lane = threadIdx.x % r1e::WAVE;
    Fr29 acc = r1e::range_sum(M, z, M.row_ptr[row], M.row_ptr[row + 1], lane, r1e::WAVE);
#pragma unroll
    for (int off = r1e::WAVE / 2; off >= 1; off >>= 1) {
        Fr29 o;
#pragma unroll
        for (int i = 0; i < fr29::N; ++i) o.l[i] = (uint32_t)__shfl_down((int)acc.l[i], off);
        acc = r1e::add_mod(acc, o);
    }
    if (lane == 0) out[row] = fr29::repack_to32(acc);
}

// *first = the smallest row with a * b != c (~0 on entry)
__global__ void __launch_bounds__(256) r1cs_sat_kernel(const Fr* __restrict__ a, const Fr* __restrict__ b, const Fr* __restrict__ c, uint64_t n_rows,
                                                       unsigned long long* __restrict__ first) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    if (!r1e::row_holds(a[i], b[i], c[i])) atomicMin(first, (unsigned long long)i);
}

// groth16.hip / bzk_r1cs_eval_dev: the evaluation of the outputs that are not null, in stream order; arguments already checked
int32_t r1cs_eval_enqueue(bzk_ctx* ctx, const bzk_r1cs_mats* m, const void* z_dev, void* a_dev, void* b_dev, void* c_dev, uint64_t pad_rows) {
    void* const out[3] = {a_dev, b_dev, c_dev};
    const uint64_t n_pad = pad_rows - m->n_rows;
    uint64_t gx = 0;
    for (int k = 0; k < 3; ++k) {
        if (!out[k]) continue;
        const uint64_t short_blocks = ((uint64_t)m->n_short[k] + n_pad + EVAL_BLOCK - 1) / EVAL_BLOCK;  // as the kernel computes them
        gx = std::max<uint64_t>(gx, short_blocks + m->long_blocks[k]);
    }
    if (!gx) return BZK_OK;
    if (gx > 0x7fffffffull) {
        ctx->last_error = "r1cs_eval: " + std::to_string(pad_rows) + " padded rows exceed one launch";
        return BZK_E_ARG;
    }
    BZK_LAUNCH(ctx, "r1cs_eval", r1cs_eval_kernel, dim3((unsigned)gx, 3), dim3(EVAL_BLOCK), 0, m->d_mats, (const Fr*)z_dev, (Fr*)a_dev, (Fr*)b_dev,
               (Fr*)c_dev, pad_rows);
    return BZK_OK;
}
// *first_dev = the first row of n_rows with a * b != c, ~0 where all hold; in stream order
int32_t r1cs_sat_enqueue(bzk_ctx* ctx, const void* a_dev, const void* b_dev, const void* c_dev, uint64_t n_rows, uint64_t* first_dev) {
    BZK_HIP(ctx, hipMemsetAsync(first_dev, 0xff, 8, ctx->stream));
    if (!n_rows) return BZK_OK;
    BZK_LAUNCH(ctx, "r1cs_sat", r1cs_sat_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, (const Fr*)a_dev, (const Fr*)b_dev,
               (const Fr*)c_dev, n_rows, (unsigned long long*)first_dev);
    return BZK_OK;
}
void r1cs_mats_shape(const bzk_r1cs_mats* m, uint64_t* n_rows, uint64_t* n_vars, int* device) {
    *n_rows = m->n_rows;
    *n_vars = (uint64_t)m->n_in + m->n_aux;
    *device = m->owner ? m->device : -1;
}

}  // namespace bzk

// a call without a context leaves its refusal where bzk_last_error(NULL) finds it
static int32_t refuse(bzk_ctx* ctx, const std::string& why) {
    if (ctx) ctx->last_error = why;
    else bzk::set_null_ctx_error(why);
    return BZK_E_ARG;
}

using bzk::EVAL_BLOCK;

extern "C" {

int32_t bzk_r1cs_mats_load(bzk_ctx* ctx, const bzk_csr* A, const bzk_csr* B, const bzk_csr* C, uint32_t n_in, uint32_t n_aux, bzk_r1cs_mats** out) {
    if (!out) return BZK_E_ARG;
    *out = nullptr;
    const bzk_csr* const M[3] = {A, B, C};
    std::string err;
    if (!r1e::validate(M, n_in, n_aux, err)) return refuse(ctx, err);
    bzk_r1cs_mats* m = new (std::nothrow) bzk_r1cs_mats();
    if (!m) return BZK_E_ALLOC;
    try {
        r1e::build(M, n_in, n_aux, m->host);
    } catch (const std::bad_alloc&) {
        delete m;
        return BZK_E_ALLOC;
    }
    const r1e::HostMats& h = m->host;
    m->owner = ctx;
    m->n_in = n_in;
    m->n_aux = n_aux;
    m->n_rows = h.n_rows;
    m->n_dict = h.n_dict;
    m->n_pm1 = h.n_pm1;
    for (int k = 0; k < 3; ++k) {
        m->nnz[k] = h.nnz(k);
        m->n_short[k] = (uint32_t)h.short_rows[k].size();
        m->long_blocks[k] = (uint32_t)((h.long_rows[k].size() + EVAL_BLOCK / r1e::WAVE - 1) / (EVAL_BLOCK / r1e::WAVE));
    }
    if (!ctx) {
        m->bytes = h.bytes();
        *out = m;
        return BZK_OK;
    }
    // one device allocation: three Mat records, then the dictionary and every matrix's arrays, each 256-byte aligned
    (void)hipSetDevice(ctx->device);
    m->device = ctx->device;
    struct Part { const std::vector<uint32_t>* v; size_t off; };
    std::vector<Part> parts;
    size_t end = 3 * sizeof(r1e::Mat);
    auto place = [&](const std::vector<uint32_t>& v) {
        end = (end + 255) & ~(size_t)255;
        parts.push_back({&v, end});
        end += v.size() * 4;
        return parts.back().off;
    };
    const size_t dict_at = place(h.dict);
    size_t at[3][5];
    for (int k = 0; k < 3; ++k) {
        at[k][0] = place(h.row_ptr[k]);
        at[k][1] = place(h.col[k]);
        at[k][2] = place(h.cidx[k]);
        at[k][3] = place(h.short_rows[k]);
        at[k][4] = place(h.long_rows[k]);
    }
    auto fail = [&](int32_t st, const std::string& why) {
        ctx->last_error = why;
        (void)hipGetLastError();
        if (m->dev) (void)hipFree(m->dev);
        delete m;
        return st;
    };
    hipError_t e = hipMalloc(&m->dev, end);
    if (e != hipSuccess) {
        m->dev = nullptr;
        return fail(BZK_E_ALLOC, std::string("r1cs_mats_load: ") + hipGetErrorString(e));
    }
    char* const base = (char*)m->dev;
    r1e::Mat recs[3];
    for (int k = 0; k < 3; ++k) {
        auto p = [&](size_t off) { return (const uint32_t*)(base + off); };
        recs[k] = r1e::Mat{p(at[k][0]), p(at[k][1]), p(at[k][2]), p(dict_at), p(at[k][3]), p(at[k][4]),
                           (uint32_t)h.short_rows[k].size(), (uint32_t)h.long_rows[k].size(), h.n_rows};
    }
    e = hipMemcpyAsync(base, recs, sizeof(recs), hipMemcpyHostToDevice, ctx->stream);
    for (size_t i = 0; i < parts.size() && e == hipSuccess; ++i)
        if (!parts[i].v->empty()) e = hipMemcpyAsync(base + parts[i].off, parts[i].v->data(), parts[i].v->size() * 4, hipMemcpyHostToDevice, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);  // always: the copies read `recs` and the host form
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(BZK_E_DEVICE, std::string("r1cs_mats_load: ") + hipGetErrorString(e));
    m->d_mats = (const r1e::Mat*)base;
    m->bytes = end;
    m->host = r1e::HostMats();  // the device copy is the resident one
    *out = m;
    return BZK_OK;
}

int32_t bzk_r1cs_mats_from_r1cs(bzk_ctx* ctx, const bzk_r1cs* r, bzk_r1cs_mats** out) {
    if (!out) return BZK_E_ARG;
    *out = nullptr;
    uint64_t info[9];
    if (!r || bzk_r1cs_info(r, info) != BZK_OK) return refuse(ctx, "r1cs_mats_from_r1cs: no instance");
    bzk_csr M[3];
    for (int k = 0; k < 3; ++k) {
        uint64_t bv = 0, bc = 0, bp = 0;
        M[k].val = (const uint8_t*)bzk_r1cs_data(r, 6 + k, &bv);
        M[k].col = (const uint32_t*)bzk_r1cs_data(r, 9 + k, &bc);
        M[k].row_ptr = (const uint32_t*)bzk_r1cs_data(r, 12 + k, &bp);
        if (bp < 4 || bp != (info[2] + 1) * 4 || bc * 8 != bv)
            return refuse(ctx, "r1cs_mats_from_r1cs: the instance holds no matrices (synthesize it with record_matrices)");
        M[k].n_rows = info[2];
    }
    return bzk_r1cs_mats_load(ctx, &M[0], &M[1], &M[2], (uint32_t)info[0], (uint32_t)info[1], out);
}

void bzk_r1cs_mats_free(bzk_ctx* ctx, bzk_r1cs_mats* m) {
    if (!m) return;
    if (m->dev) {
        (void)hipSetDevice(m->device);
        if (ctx) (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(m->dev);
    }
    delete m;
}

int32_t bzk_r1cs_mats_info(const bzk_r1cs_mats* m, uint64_t info[8]) {
    if (!m || !info) return BZK_E_ARG;
    info[0] = m->n_rows;
    info[1] = (uint64_t)m->n_in + m->n_aux;
    info[2] = m->nnz[0];
    info[3] = m->nnz[1];
    info[4] = m->nnz[2];
    info[5] = m->n_dict;
    info[6] = m->bytes;
    info[7] = 0;
    return BZK_OK;
}

static int32_t eval_call_checks(bzk_ctx* ctx, const bzk_r1cs_mats* m, const void* z, uint64_t n_vars, const char* who) {
    if (!m) return refuse(ctx, std::string(who) + ": no matrices");
    if (!z) return refuse(ctx, std::string(who) + ": z is NULL");
    if (n_vars != (uint64_t)m->n_in + m->n_aux)
        return refuse(ctx, std::string(who) + ": the witness has " + std::to_string(n_vars) + " variables, the matrices " + std::to_string((uint64_t)m->n_in + m->n_aux));
    if (ctx && (!m->owner || m->device != ctx->device))
        return refuse(ctx, std::string(who) + (m->owner ? ": the matrices are resident on another device" : ": the matrices were loaded without a context (host memory)"));
    if (!ctx && m->owner) return refuse(ctx, std::string(who) + ": the matrices are resident on a device, the host-thread route needs a handle loaded with ctx = NULL");
    return BZK_OK;
}

int32_t bzk_r1cs_eval_dev(bzk_ctx* ctx, const bzk_r1cs_mats* m, const void* z_dev, uint64_t n_vars, void* az_dev, void* bz_dev, void* cz_dev,
                          uint64_t pad_rows) {
    if (!ctx) return BZK_E_ARG;
    BZK_TRY(eval_call_checks(ctx, m, z_dev, n_vars, "r1cs_eval_dev"));
    if (pad_rows < m->n_rows) return refuse(ctx, "r1cs_eval_dev: pad_rows " + std::to_string(pad_rows) + " < " + std::to_string(m->n_rows) + " rows");
    (void)hipSetDevice(ctx->device);
    return bzk::r1cs_eval_enqueue(ctx, m, z_dev, az_dev, bz_dev, cz_dev, pad_rows);
}

int32_t bzk_r1cs_eval(bzk_ctx* ctx, const bzk_r1cs_mats* m, const uint8_t* z, uint64_t n_vars, uint8_t* az, uint8_t* bz, uint8_t* cz, int64_t* first_unsat) {
    BZK_TRY(eval_call_checks(ctx, m, z, n_vars, "r1cs_eval"));
    uint8_t* const out[3] = {az, bz, cz};
    const uint64_t n_rows = m->n_rows;
    if (!ctx) {
        // the host-thread route: row_eval per row, blocks of rows per task; the check needs all three evaluations, kept per block
        const Fr* zz = (const Fr*)z;
        r1e::Mat M[3];
        for (int k = 0; k < 3; ++k) M[k] = m->host.view(k);
        std::atomic<uint64_t> first(~0ull);
        constexpr uint64_t ROWS = 512;
        bzk::host_for_each((n_rows + ROWS - 1) / ROWS, bzk::host_default_threads(), [&](uint64_t blk) {
            const uint64_t r0 = blk * ROWS, r1 = std::min(n_rows, r0 + ROWS);
            for (uint64_t i = r0; i < r1; ++i) {
                Fr v[3];
                for (int k = 0; k < 3; ++k) {
                    if (!out[k] && !first_unsat) continue;
                    v[k] = r1e::row_eval(M[k], zz, i);
                    if (out[k]) memcpy(out[k] + i * 32, v[k].l, 32);
                }
                if (first_unsat && !r1e::row_holds(v[0], v[1], v[2])) {
                    uint64_t cur = first.load();
                    while (i < cur && !first.compare_exchange_weak(cur, i)) {}
                }
            }
        });
        if (first_unsat) *first_unsat = first.load() == ~0ull ? -1 : (int64_t)first.load();
        return BZK_OK;
    }
    (void)hipSetDevice(ctx->device);
    // the call's workspace: the witness, the evaluations that are wanted (all three for the check) and the check's word
    Fr *dz = nullptr, *dv[3] = {nullptr, nullptr, nullptr};
    uint64_t* dfirst = nullptr;
    bzk::WsLayout ws("r1cs_eval");
    ws.take(dz, n_vars);
    for (int k = 0; k < 3; ++k)
        if (out[k] || first_unsat) ws.take(dv[k], n_rows);
    if (first_unsat) ws.take(dfirst, 1);
    BZK_TRY(ws.commit(ctx));
    BZK_HIP(ctx, hipMemcpyAsync(dz, z, n_vars * 32, hipMemcpyHostToDevice, ctx->stream));
    uint64_t first = ~0ull;
    int32_t st = bzk::r1cs_eval_enqueue(ctx, m, dz, dv[0], dv[1], dv[2], n_rows);
    if (st == BZK_OK && first_unsat) st = bzk::r1cs_sat_enqueue(ctx, dv[0], dv[1], dv[2], n_rows, dfirst);
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3 && st == BZK_OK && e == hipSuccess; ++k)
        if (out[k] && n_rows) e = hipMemcpyAsync(out[k], dv[k], n_rows * 32, hipMemcpyDeviceToHost, ctx->stream);
    if (st == BZK_OK && e == hipSuccess && first_unsat) e = hipMemcpyAsync(&first, dfirst, 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);  // always: the copies name the caller's arrays and this frame
    if (st != BZK_OK) return st;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        ctx->last_error = std::string("r1cs_eval: ") + hipGetErrorString(e);
        return BZK_E_DEVICE;
    }
    if (first_unsat) *first_unsat = first == ~0ull ? -1 : (int64_t)first;
    return BZK_OK;
}

}  // extern "C"
