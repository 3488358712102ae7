// Internal plumbing of libbzk: context, error handling, workspace, per-kernel event timing.
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <string.h>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bzk.h"
#include "bzk_ws.h"
#include "bzk_mpn_wire.h"  // TxSoA / WdSoA / DpSoA and the mpn_*_verify_run of eddsa.hip

struct bzk_prof_rec {
    const char* name;
    hipEvent_t a, b;
};

// An instance's assignment resident in HBM (bzk_r1cs_stage, groth16.hip): z | A.z | B.z | C.z as the prover reads them, complete - the deferred-value
// program, if the instance had one, has run behind the uploads on the staging context's stream; `ready` marks the end of that work
struct bzk_staged {
    bzk_ctx* owner = nullptr;
    void* buf = nullptr;          // one allocation: z (n_vars) | az | bz | cz (n_rows each), 32-byte scalars
    size_t cap = 0;               // bytes behind buf
    uint64_t n_vars = 0, n_rows = 0;
    hipEvent_t ready = nullptr;
    uint32_t* flags_host = nullptr;  // pinned: wf::FLAG_* of the program (0 without one), valid once `ready` has completed
    void* z() const { return buf; }
    void* ev(int k) const { return (char*)buf + (n_vars + (uint64_t)k * n_rows) * 32; }
};

struct bzk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string last_error;
    int32_t last_refusal = 0;  // BZK_REFUSE_*: what the last BZK_E_ARG of a bzk_state_* call stands for (bzk_last_refusal)
    bool prof = false;
    std::string prof_only;  // non-empty: only launches whose label contains it get event pairs (bzk_prof_filter)
    std::vector<bzk_prof_rec> recs;
    // grow-only scratch buffer reused across calls: carved by one bzk::WsLayout per call (bzk_ws.h), never addressed directly
    void* ws = nullptr;
    size_t ws_bytes = 0;
    const char* ws_live = nullptr;  // the call whose committed WsLayout is in scope (the slab must not move under it); cleared by its destructor
    // pinned host staging (small results)
    void* pinned = nullptr;
    size_t pinned_bytes = 0;
    // device-resident Poseidon constants per width t (index t), Montgomery, rc then mds
    void* poseidon_dev[18] = {};
    // MSM tuning overrides (0 = automatic); settable through env BZK_MSM_C / BZK_MSM_CHUNK
    int msm_c_override = 0;
    int msm_chunk_override = 0;
    bool msm_no_endo = false;  // env BZK_MSM_NO_ENDO=1 (and the device groups' contexts): resident base sets without endomorphism images, plain windows
    int msm_reduce2 = 0;  // env BZK_MSM_REDUCE2: 1 forces the two-level bucket reduction, -1 forbids it, 0 = per call (BZK_F_THROUGHPUT)
    bool debug = false;  // env BZK_DEBUG=1: synchronise + log after every launch (hang localisation)
    // NTT twiddle cache: per log_n, forward and inverse tables
    void* ntt_tw[33][2] = {};
    // lanes: child contexts (own stream, workspace, pinned staging) for independent sub-jobs of one call that
    // should overlap on the device - the five MSMs of a Groth16 proof.  Created on first use, owned by the parent.
    std::vector<bzk_ctx*> lanes;
    std::vector<struct bzk_lane_thread*> lane_threads;  // one persistent host thread per lane (ctx.hip: lane_post / lane_wait)
    // round 6 (run 18): child contexts of ONE stand-alone MSM call whose windows run as several ranges in flight (msm_impl.cuh msm_run_split): the
    // front chain of one range hides under the accumulation of another, the tails of one under the accumulation of the next.  Own stream + workspace
    // each, created on first use, owned by the parent; `is_part` marks such a child (it never splits again).  split_terms: device staging of the terms
    // the ranges leave (W x terms per set x 192 B), split_ev: the fork event recorded on the parent's stream
    // msm_split: ranges per call (0 = the library default, 1 = off), msm_split_min_log: smallest log2(n) that splits, msm_split_prio: children at the highest
    // stream priority - read from env BZK_MSM_SPLIT / BZK_MSM_SPLIT_MIN_LOG / BZK_MSM_SPLIT_PRIO when the context is created (tests and A/B runs)
    std::vector<bzk_ctx*> parts;
    int msm_split = 0, msm_split_min_log = 0, msm_split_prio = -1;
    int msm_front = 0;  // env BZK_MSM_FRONT=sort|partition: how a plain MSM call buckets its pairs (0 = msm_front_plan's measured choice, 1 = radix sort, 2 = partition passes; A/B)
    int msm_split_cuts[4] = {0, 0, 0, 0};  // env BZK_MSM_SPLIT_CUTS="a,b[,c[,d]]": windows per range, highest range first (A/B runs; used when they add up to W)
    bool is_part = false, split_active = false;
    // env BZK_MSM_BASES_TABLE / BZK_MSM_BASES_TABLE_C (msm_impl.cuh msm_bases_table_plan): -1 = a resident G1 set of 2^19 < n <= 2^20 points is loaded with a
    // c = 20 window table, 0 = never, 1 = every G1 set whose table fits; the window of the table, 11 .. 20 (0 = 20; tests reach every shape at small n).
    // is_child: a lane or a window-range child - its calls never take a set's table; msm_split_env: some BZK_MSM_SPLIT* variable was set when the context was created
    int msm_bases_table = -1, msm_bases_table_c = 0;
    bool is_child = false, msm_split_env = false;
    // env BZK_MSM_BITSUM_PLAIN=0: a table call's one bucket set leaves its terms in the paired layout of every other caller (msm_impl.cuh msm_bitsum_quad_kernel; A/B runs, tests)
    bool msm_bitsum_plain = true;
    void* split_terms = nullptr;
    size_t split_terms_bytes = 0;
    void* split_conv = nullptr;  // internal form of the raw bases of a split call (msm_entry_dev), grow-only; released by bzk_ctx_trim
    size_t split_conv_bytes = 0;
    hipEvent_t split_ev = nullptr;
    bool no_coop = false;  // env BZK_NO_COOP=1: never use the cooperative (8 lanes per node) Poseidon kernel (A/B runs)
    bool timing = false;  // env BZK_TIMING=1: host-side phase timings of bzk_groth16_prove on stderr
    hipEvent_t ev_z = nullptr;  // "assignment staged" event of bzk_groth16_prove: created on first use, destroyed with the ctx
    // side stream of one MSM call: work that the bucket pipeline does not depend on until the accumulation (the per-call base
    // conversion) runs here beside digits / sort; fork / join through the two events.  Created on first use.
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // env BZK_PROVE_H_PRIO=1 (A/B runs, measured neutral): highest-priority side stream of bzk_groth16_prove for the h polynomial
    // (evaluations staged + seven transforms).  Created on first use.
    hipStream_t hprio = nullptr;
    hipEvent_t ev_h = nullptr;
    // round 6: the SATURATING kernels of an MSM (accumulation, folds, bucket reduction) on a lowest-priority side stream, so that the short kernels of
    // OTHER streams' MSMs (digits, sorts, boundaries - the chain that gates their next accumulation) are not starved beside them (msm_impl.cuh HeavyScope)
    hipStream_t heavy = nullptr;
    hipEvent_t ev_heavy_in = nullptr, ev_heavy_out = nullptr;
    bool heavy_tried = false;
    bool heavy_force = false;  // a later window range of a split call (msm_run_split, priority mode 2): HeavyScope applies whatever BZK_MSM_HEAVY_PRIO says
    void* eddsa_tab = nullptr;  // eddsa.hip: the signature verifier's fixed-base table (multiples of Jubjub's BASE, 29-bit form), built on first use
    void* ed25519_tab = nullptr;  // eddsa.hip: the Ed25519 verifier's fixed-base table (j 16^i B, bzk_ed25519.cuh base_table_build), built on first use
    void* wf_state = nullptr;  // witfill.hip: device copies of the deferred-witness programs, dense Poseidon constants, scratch (witfill_free)
    // bzk_r1cs_stage: staged assignments handed back by bzk_staged_free (possibly from another thread: the prover's), kept for the next call
    std::mutex staged_mu;
    std::vector<bzk_staged*> staged_pool;
};

#define BZK_HIP(ctx, call)                                                                  \
    do {                                                                                    \
        hipError_t e__ = (call);                                                            \
        if (e__ != hipSuccess) {                                                            \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e__);         \
            return BZK_E_DEVICE;                                                            \
        }                                                                                   \
    } while (0)

#define BZK_TRY(expr)                 \
    do {                              \
        int32_t s__ = (expr);         \
        if (s__ != BZK_OK) return s__; \
    } while (0)

// the device operations of a staged call (bzk_stage.h Stage<StreamOps>) on the context's stream
struct StreamOps {
    bzk_ctx* ctx;
    int32_t up(void* dev, const void* host, size_t bytes) const {
        BZK_HIP(ctx, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
        return BZK_OK;
    }
    int32_t down(void* host, const void* dev, size_t bytes) const {
        BZK_HIP(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        return BZK_OK;
    }
    int32_t zero(void* dev, size_t bytes) const {
        BZK_HIP(ctx, hipMemsetAsync(dev, 0, bytes, ctx->stream));
        return BZK_OK;
    }
    int32_t sync() const {
        BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return BZK_OK;
    }
};

// groth16.hip hooks used by setup.hip
int32_t bzk_params_alloc_internal(bzk_ctx* ctx, const bzk_params_desc* d, bzk_params** out);
void bzk_params_buffers_internal(bzk_params* p, void** h, void** l, void** a, void** b_g1, void** b_g2);
void bzk_params_set_vk_internal(bzk_params* p, const uint8_t vk[870]);

namespace bzk {

bzk_ctx* ctx_lane(bzk_ctx* ctx, size_t i);                // i-th child context (nullptr on failure)
bzk_ctx* ctx_part(bzk_ctx* ctx, size_t i, bool high_prio); // i-th window-range child of a split MSM call (nullptr on failure)
int32_t pinned_reserve(bzk_ctx* ctx, size_t bytes);
// runs `job` on the persistent host thread of lane i (created on first use, bound to the ctx's device); lane_wait blocks until that
// job has returned.  One job per lane at a time.
void lane_post(bzk_ctx* ctx, size_t i, std::function<void()> job);
void lane_wait(bzk_ctx* ctx, size_t i);

void witfill_free(bzk_ctx* ctx);  // witfill.hip
// eddsa.hip: ok_dev[i] = verdict of signature i; device pointers, enqueued on the context's stream under the launch label "jubjub_verify"
int32_t jubjub_verify_launch(bzk_ctx* ctx, const void* pub_xy_dev, const void* msg_dev, const void* sig_dev, uint64_t n, void* ok_dev);
// eddsa.hip: xy_dev[i] = x | y of key i (zeros where it does not decompress), ok_dev[i] = 1 / 0; launch label "jubjub_decompress"
int32_t jubjub_decompress_launch(bzk_ctx* ctx, const void* x_dev, const void* odd_dev, uint64_t n, void* xy_dev, void* ok_dev);
// eddsa.hip: SHA3-256 of message i = data_dev[begin[i] - base .. end[i] - base), the 32 bytes at blank[i] inside it (blank_dev may be null) absorbed
// as zeros; digest_dev (n x 32) and scalar_dev (n x 32: hash_to_scalar) may each be null; launch label "sha3_256"
int32_t sha3_256_launch(bzk_ctx* ctx, const void* data_dev, const void* begin_dev, const void* end_dev, uint64_t base, const void* blank_dev,
                        uint64_t n, void* digest_dev, void* scalar_dev);
// eddsa.hip: the Ed25519 verifier's fixed-base table on the device (built on the context's first use)
int32_t ed25519_table_dev(bzk_ctx* ctx, const uint32_t** out);
// verify.hip: the batched Groth16 verifier as a stage of another call.  g16v_declare adds the verifier's buffers for up to n proofs per launch
// round to the CALLER's layout; after the caller's commit, g16v_enqueue runs n proofs of one valid prepared key (device pointers, stream order;
// `up` must outlive the work; sync: wait for it).  g16v_host_run: the same per-proof functions on host threads (every verdict 0 for an invalid key).
namespace hp {
struct KeyHost;
struct KeyUpload;
}  // namespace hp
struct G16vBufs {
    uint32_t *slab = nullptr, *flags = nullptr, *sc = nullptr;
    uint8_t* dkey = nullptr;
    uint32_t stride = 0;
};
void g16v_declare(WsLayout& ws, G16vBufs& b, uint32_t n_inputs, uint64_t n, size_t key_bytes);
int32_t g16v_enqueue(bzk_ctx* ctx, const G16vBufs& b, const hp::KeyHost& K, const hp::KeyUpload& up, const uint8_t* inputs_dev,
                     const uint8_t* proofs_dev, uint64_t n, uint8_t* ok_dev, bool sync);
void g16v_host_run(const hp::KeyHost& K, const uint8_t* inputs, const uint8_t* proofs, uint64_t n, uint8_t* ok);
// verify_keys.hip: the same verifier over GROUPS of proofs, a key per group, in one set of launches per round of 2^16 lanes (every group padded to
// whole blocks of 64).  A group on the device path has a valid prepared key of at most 16 inputs and count > 0; K, up and count are what
// g16k_declare reads, the three pointers are set before g16k_enqueue: device pointers to the group's rows - or, `staged`, HOST pointers to its
// inputs and proofs, which go up round by round through staging buffers the declaration adds (ok stays a device pointer).  g16k_declare cuts the
// rounds and adds the verifier's buffers, the keys' uploads, the segment records and the block table to the CALLER's layout; after the caller's
// commit g16k_enqueue runs on it in stream order (`up`, the groups and `b` must outlive the work; sync: wait for it).  g16k_host_run: the same
// per-proof functions on host threads, all groups' rows in one task loop (host pointers; every verdict of an invalid key 0; `up` is not read).
struct G16kGroup {
    const hp::KeyHost* K = nullptr;
    const hp::KeyUpload* up = nullptr;
    uint64_t count = 0;
    const uint8_t *inputs = nullptr, *proofs = nullptr;
    uint8_t* ok = nullptr;
};
struct G16kSeg {   // the rows [first, first + rows) of a group: its part of one round, from block `block0` of the round on
    uint32_t group, rows;
    uint64_t first;
    uint32_t block0;
    size_t in_at;  // staged: where its inputs lie in the round's staging buffer
};
struct G16kBufs {
    uint32_t *slab = nullptr, *flags = nullptr, *sc = nullptr;
    uint8_t *dkeys = nullptr, *dsegs = nullptr, *dblocks = nullptr, *din = nullptr, *dpr = nullptr;
    uint32_t stride = 0;                          // lanes of the largest round
    uint64_t n_blocks = 0;
    std::vector<size_t> key_at;                   // per group: its key's upload in dkeys
    std::vector<G16kSeg> segs;                    // in lane order
    std::vector<uint32_t> round_at, round_blocks; // round r: segments [round_at[r], round_at[r + 1]), round_blocks[r] blocks
    std::vector<uint8_t> hsegs, hblocks;          // the host images of dsegs and dblocks (g16k_enqueue)
};
void g16k_declare(WsLayout& ws, G16kBufs& b, const std::vector<G16kGroup>& groups, bool staged);
int32_t g16k_enqueue(bzk_ctx* ctx, G16kBufs& b, const std::vector<G16kGroup>& groups, bool staged, bool sync);
void g16k_host_run(const std::vector<G16kGroup>& groups);
// subgroup.hip: the first of n finite raw points (G1 96 B, G2 192 B) whose subgroup verdict is not 1: *idx (n: none) and *code.  ctx = NULL: host threads
// on host records; on_device: the records already are in device memory.  sg_host_one: the verdict of one record on the host
int32_t sg_first_bad(bzk_ctx* ctx, const char* who, bool g2, const uint8_t* pts, bool on_device, uint64_t n, uint64_t* idx, uint8_t* code);
uint8_t sg_host_one(bool g2, const uint8_t* raw);
// r1cs_eval.hip: the launches behind bzk_r1cs_eval_dev as a stage of bzk_groth16_prove_witness, in stream order, arguments checked by the caller.
// r1cs_eval_enqueue: A.z, B.z, C.z of device-resident matrices into a / b / c (a null one is skipped), rows n_rows .. pad_rows written as zero;
// r1cs_sat_enqueue: *first_dev = the first of n_rows rows with a * b != c, ~0 where every row holds; r1cs_mats_shape: *device = -1 for a handle in host memory
int32_t r1cs_eval_enqueue(bzk_ctx* ctx, const bzk_r1cs_mats* m, const void* z_dev, void* a_dev, void* b_dev, void* c_dev, uint64_t pad_rows);
int32_t r1cs_sat_enqueue(bzk_ctx* ctx, const void* a_dev, const void* b_dev, const void* c_dev, uint64_t n_rows, uint64_t* first_dev);
void r1cs_mats_shape(const bzk_r1cs_mats* m, uint64_t* n_rows, uint64_t* n_vars, int* device);
std::string& null_ctx_error();                   // ctx.hip: what bzk_last_error(NULL) answers on this thread
void set_null_ctx_error(const std::string& e);
int32_t ntt_run(bzk_ctx* ctx, void* data_dev, uint32_t log_n, int inverse, int coset);  // ntt.hip
int32_t ntt_h_chain(bzk_ctx* ctx, void* a, void* b, void* c, uint32_t log_m);              // ntt.hip: the h polynomial's 7 transforms, fused
// msm_g1.hip / msm_g2.hip: windows [w_begin, w_end) (w_end < 0: all) of an MSM over a resident base set (or raw bases when `bases` is
// null); the window sums stay in DEVICE memory at d_win as standard-limb XYZZ points (G1 192 B, G2 384 B each), in stream order,
// nothing is read back.  info = {c, w_total, w_begin, w_end, terms per bucket set (0: window sums; G1 since round 6: msm_g1_window_terms)}.  *_horner_packed: host Horner sum_k 2^(c (w0 + k)) S[k] -> packed point
int32_t msm_g1_windows_dev(bzk_ctx* ctx, const bzk_msm_bases* bases, const void* bases_raw, const void* scalars, uint64_t n, uint32_t flags,
                           int w_begin, int w_end, void* d_win, int32_t info[5]);
int32_t msm_g2_windows_dev(bzk_ctx* ctx, const bzk_msm_bases* bases, const void* bases_raw, const void* scalars, uint64_t n, uint32_t flags,
                           int w_begin, int w_end, void* d_win, int32_t info[5]);
// msm_g1.hip: bzk_msm_g1_bases_load_dev without a window table, whatever BZK_MSM_BASES_TABLE says - for the loaders whose calls can never take one
// (the prover's queries: throughput-flagged or de-duplicated; the device groups: window ranges)
int32_t msm_g1_bases_load_plain(bzk_ctx* ctx, const void* bases_dev, uint64_t n, bzk_msm_bases** out);
int msm_window_bits(uint64_t n);
int msm_g1_window_terms(uint64_t n);  // 0: a window-range G1 call leaves window sums at d_win; k > 0: the k terms of every bucket set (info[4] of the call agrees)
int32_t g1_horner_terms_packed(const void* T, int count, int c, int w0, uint8_t* out);
int32_t g1_horner_packed(const void* S, int count, int c, int w0, uint8_t* out);
int32_t g2_horner_packed(const void* S, int count, int c, int w0, uint8_t* out);
// an environment switch: set and not "0" (one getenv: the value is read from the pointer it was tested on)
static inline bool env_on(const char* name) {
    const char* e = getenv(name);
    return e && atoi(e) != 0;
}

// A schedule of Poseidon hashes over one value array (state.hip): values [0, n_up) are uploaded 32-byte scalars, group g's outputs
// follow in group order.  Groups run one batched launch each, in order, so a group may consume anything uploaded or produced by an
// earlier group.  Used by the general state compress and by the device path of the MPN witness builders (mpn.hip).
struct HashGroup {
    uint32_t arity = 0;
    std::vector<uint32_t> in;  // count * arity value ids (already resolved: < n_up + outputs of earlier groups)
    uint32_t count() const { return arity ? (uint32_t)(in.size() / arity) : 0; }
};
// uploaded: n_up x 32 B Montgomery scalars; hashed_out receives sum(count) x 32 B in group order
int32_t hash_plan_run(bzk_ctx* ctx, const uint8_t* uploaded, uint64_t n_up, const std::vector<HashGroup>& groups, std::vector<uint8_t>& hashed_out);

struct ProfScope {
    bzk_ctx* ctx;
    hipEvent_t a = nullptr, b = nullptr;
    const char* name;
    ProfScope(bzk_ctx* c, const char* n) : ctx(c), name(n) {
        if (ctx->prof && (ctx->prof_only.empty() || strstr(n, ctx->prof_only.c_str()))) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            (void)hipEventRecord(a, ctx->stream);
        }
    }
    ~ProfScope() {
        if (a) {
            (void)hipEventRecord(b, ctx->stream);
            ctx->recs.push_back({name, a, b});
        }
    }
};

// launch + error check; `name` must be a string literal (kept by pointer)
#define BZK_LAUNCH(ctx, name, kernel, grid, block, shmem, ...)                                      \
    do {                                                                                            \
        {                                                                                           \
            bzk::ProfScope ps__(ctx, name);                                                         \
            hipLaunchKernelGGL(kernel, grid, block, shmem, (ctx)->stream, __VA_ARGS__);              \
        }                                                                                           \
        hipError_t e__ = hipGetLastError();                                                         \
        if (e__ == hipSuccess && (ctx)->debug) {                                                    \
            fprintf(stderr, "[bzk] launched %s ...", name);                                         \
            fflush(stderr);                                                                         \
            e__ = hipStreamSynchronize((ctx)->stream);                                              \
            fprintf(stderr, " %s\n", e__ == hipSuccess ? "done" : hipGetErrorString(e__));          \
            fflush(stderr);                                                                         \
        }                                                                                           \
        if (e__ != hipSuccess) {                                                                    \
            (ctx)->last_error = std::string("launch ") + name + ": " + hipGetErrorString(e__);      \
            return BZK_E_DEVICE;                                                                    \
        }                                                                                           \
    } while (0)

}  // namespace bzk
