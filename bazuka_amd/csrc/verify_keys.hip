// Batched Groth16 verification of proofs of SEVERAL keys in one set of launches (bzk_groth16_verify_batch_keys, bzk_groth16_verify_groups_dev, and
// the verifier stage of bzk_contract_updates_check).  verify.hip's call costs one lane's chain of dependent products (about 53 ms) per KEY, however
// few proofs the key has; a block carries proofs of three keys.  Here the lanes of all groups lie side by side: group after group, each padded to
// a whole block of 64, so every block - and so every wavefront - belongs to one key, reads its key's tables at one address per wave as
// verify.hip's kernels do, and never diverges on n_inputs.  The per-proof arithmetic is bzk_pairing28.cuh's prepare_one / miller_one /
// finalexp_one, unchanged; this file holds the round cut, the three kernels (the same thin wrappers, finding their key through a block table),
// the host side (keys prepared side by side on the host threads, the stable grouping of the host form, the scatter of verdicts) and the entries.
//
// A round is at most G16K_ROUND lanes (1 024 blocks) on one slab.  The cut walks the groups in order and gives every (group, round) intersection
// one SEGMENT: a record {key view, inputs, proofs, ok, count} whose pointers name the segment's first row, so a group that straddles a round
// boundary has two records of the same key and neither kernel nor host ever subtracts a round's origin.  The block table holds per block its
// segment and the index of its first row within the segment; a round's launches get the table from the round's first block on.
#include <memory>

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

constexpr int G16K_BLOCK = 64;
constexpr uint64_t G16K_ROUND = (uint64_t)1 << 16;        // lanes per round of launches (verify.hip's G16V_ROUND); a later round reuses the slab
constexpr uint32_t G16K_ROUND_BLOCKS = (uint32_t)(G16K_ROUND / G16K_BLOCK);
constexpr uint32_t G16K_MAX_INPUTS = 16;                  // above: the host-thread path, as in verify.hip

struct SegRec {   // one segment as the kernels read it
    KeyDev k;
    const uint8_t* inputs;
    const uint8_t* proofs;
    uint8_t* ok;
    uint32_t count;
};
struct BlockRec {
    uint32_t seg, first;   // the block's segment, and the index within it of the block's first row
};

// blocks: the round's part of the block table, so blockIdx.x counts from the round's first block and lane i is the round's lane.  The segment
// is the same for all 64 lanes: its record is read at one address per wave and the key goes on BY VALUE, as a kernel argument does in verify.hip
__global__ void __launch_bounds__(G16K_BLOCK) g16k_prepare_kernel(const SegRec* __restrict__ segs, const BlockRec* __restrict__ blocks,
                                                                  uint32_t* __restrict__ slab, uint32_t stride, uint32_t* __restrict__ sc,
                                                                  uint32_t* __restrict__ flags) {
    const BlockRec b = blocks[blockIdx.x];
    const SegRec& s = segs[b.seg];
    const uint32_t j = b.first + threadIdx.x;
    if (j >= s.count) return;
    const KeyDev k = s.k;
    const uint32_t i = blockIdx.x * G16K_BLOCK + threadIdx.x;
    flags[i] = pairing::prepare_one(Lane28{slab + i, stride}, k, s.inputs + (size_t)32 * k.n_inputs * j, s.proofs + (size_t)387 * j, sc + i, stride);
}
__global__ void __launch_bounds__(G16K_BLOCK) g16k_miller_kernel(const SegRec* __restrict__ segs, const BlockRec* __restrict__ blocks,
                                                                 uint32_t* __restrict__ slab, uint32_t stride, uint32_t* __restrict__ flags) {
    const BlockRec b = blocks[blockIdx.x];
    const SegRec& s = segs[b.seg];
    if (b.first + threadIdx.x >= s.count) return;
    const KeyDev k = s.k;
    const uint32_t i = blockIdx.x * G16K_BLOCK + threadIdx.x;
    const uint32_t f = flags[i];
    if (f & pairing::FLAG_REFUSED) return;
    flags[i] = pairing::miller_one(Lane28{slab + i, stride}, k, f);
}
// every lane writes its verdict straight to its segment's ok: no scatter pass
__global__ void __launch_bounds__(G16K_BLOCK) g16k_finalexp_kernel(const SegRec* __restrict__ segs, const BlockRec* __restrict__ blocks,
                                                                   uint32_t* __restrict__ slab, uint32_t stride,
                                                                   const uint32_t* __restrict__ flags) {
    const BlockRec b = blocks[blockIdx.x];
    const SegRec& s = segs[b.seg];
    const uint32_t j = b.first + threadIdx.x;
    if (j >= s.count) return;
    const KeyDev k = s.k;
    const uint32_t i = blockIdx.x * G16K_BLOCK + threadIdx.x;
    if (flags[i] & (pairing::FLAG_REFUSED | pairing::FLAG_DEGENERATE)) {
        s.ok[j] = 0;
        return;
    }
    s.ok[j] = pairing::finalexp_one(Lane28{slab + i, stride}, k) ? 1 : 0;
}

// the three per-lane steps of one proof over the host field
void host_one(const KeyHost& K, const uint8_t* in, const uint8_t* pr, uint8_t* ok) {
    if (!K.valid) {
        *ok = 0;
        return;
    }
    const KeyHostView k = K.view();
    HFp slab[pairing::slot::COUNT];
    thread_local std::vector<uint32_t> sc;   // the canonical scalars: grown per thread, not per proof
    if (sc.size() < (size_t)8 * K.n_inputs + 1) sc.resize((size_t)8 * K.n_inputs + 1);
    const hp::LaneH l = {slab};
    uint32_t f = pairing::prepare_one(l, k, in, pr, sc.data(), 1);
    if (!(f & pairing::FLAG_REFUSED)) f = pairing::miller_one(l, k, f);
    *ok = (f & (pairing::FLAG_REFUSED | pairing::FLAG_DEGENERATE)) ? 0 : (pairing::finalexp_one(l, k) ? 1 : 0);
}

// a call's keys, prepared side by side on the host threads: key k is prepared when use[k], uploaded when it is valid and takes the device path
struct Keys {
    std::vector<KeyHost> key;
    std::vector<std::unique_ptr<KeyUpload>> up;
    bool device(size_t k) const { return up[k] != nullptr; }
};
void prepare_keys(Keys& K, uint32_t n_keys, const uint8_t* vks, const uint64_t* vk_off, const uint32_t* n_inputs, const std::vector<uint8_t>& use,
                  bool device) {
    K.key.resize(n_keys);
    K.up.resize(n_keys);
    host_for_each(n_keys, host_default_threads(), [&](uint64_t k) {
        if (!use[k]) return;
        key_prepare(vks + vk_off[k], vk_off[k + 1] - vk_off[k], n_inputs[k], K.key[k]);
        if (device && K.key[k].valid && n_inputs[k] <= G16K_MAX_INPUTS) K.up[k].reset(new KeyUpload(K.key[k]));
    });
}
// vk_off ascending and every key at least the fixed part long
bool keys_well_formed(uint32_t n_keys, const uint64_t* vk_off) {
    for (uint32_t k = 0; k < n_keys; ++k)
        if (vk_off[k + 1] < vk_off[k] || vk_off[k + 1] - vk_off[k] < 878) return false;
    return true;
}

}  // namespace

// ---- the seam (bzk_internal.h): a caller declares the verifier's buffers for its groups in ITS layout, commits once, and enqueues
void g16k_declare(WsLayout& ws, G16kBufs& b, const std::vector<G16kGroup>& groups, bool staged) {
    b.segs.clear();
    b.round_at.assign(1, 0);
    b.round_blocks.clear();
    uint32_t used = 0, max_inputs = 0;
    size_t key_bytes = 0, in_round = 0, in_cap = 0;
    b.key_at.clear();
    for (size_t g = 0; g < groups.size(); ++g) {
        const G16kGroup& G = groups[g];
        b.key_at.push_back(key_bytes);
        key_bytes = (key_bytes + G.up->bytes.size() + WsLayout::ALIGN - 1) & ~(WsLayout::ALIGN - 1);
        max_inputs = std::max(max_inputs, G.K->n_inputs);
        for (uint64_t j = 0; j < G.count;) {
            if (used == G16K_ROUND_BLOCKS) {   // the round is full: the group goes on in the next one
                b.round_blocks.push_back(used);
                b.round_at.push_back((uint32_t)b.segs.size());
                in_cap = std::max(in_cap, in_round);
                used = 0;
                in_round = 0;
            }
            const uint32_t rows = (uint32_t)std::min<uint64_t>(G.count - j, (uint64_t)(G16K_ROUND_BLOCKS - used) * G16K_BLOCK);
            b.segs.push_back({(uint32_t)g, rows, j, used, in_round});
            used += (rows + G16K_BLOCK - 1) / G16K_BLOCK;
            in_round += (size_t)32 * G.K->n_inputs * rows;
            j += rows;
        }
    }
    b.round_blocks.push_back(used);
    b.round_at.push_back((uint32_t)b.segs.size());
    in_cap = std::max(in_cap, in_round);
    uint32_t cap_blocks = 0;
    b.n_blocks = 0;
    for (uint32_t nb : b.round_blocks) {
        cap_blocks = std::max(cap_blocks, nb);
        b.n_blocks += nb;
    }
    b.stride = cap_blocks * G16K_BLOCK;
    ws.take(b.slab, (size_t)pairing::slot::COUNT * 14 * b.stride);
    ws.take(b.flags, b.stride);
    ws.take(b.sc, (size_t)8 * max_inputs * b.stride + 1);
    ws.take(b.dkeys, key_bytes + 1);
    ws.take(b.dsegs, b.segs.size() * sizeof(SegRec) + 1);
    ws.take(b.dblocks, (size_t)b.n_blocks * sizeof(BlockRec) + 1);
    if (staged) {
        ws.take(b.din, in_cap + 1);
        ws.take(b.dpr, (size_t)387 * b.stride + 1);
    }
}

int32_t g16k_enqueue(bzk_ctx* ctx, G16kBufs& b, const std::vector<G16kGroup>& groups, bool staged, bool sync) {
    if (b.segs.empty()) return BZK_OK;
    // the segment records and the block table of all rounds, built here (the pointers are known now) and uploaded once
    std::vector<KeyDev> view(groups.size());
    for (size_t g = 0; g < groups.size(); ++g) {
        const KeyUpload& up = *groups[g].up;
        BZK_HIP(ctx, hipMemcpyAsync(b.dkeys + b.key_at[g], up.bytes.data(), up.bytes.size(), hipMemcpyHostToDevice, ctx->stream));
        view[g] = up.view(*groups[g].K, b.dkeys + b.key_at[g]);
    }
    b.hsegs.resize(b.segs.size() * sizeof(SegRec));
    b.hblocks.resize((size_t)b.n_blocks * sizeof(BlockRec));
    SegRec* hs = (SegRec*)b.hsegs.data();
    BlockRec* hb = (BlockRec*)b.hblocks.data();
    size_t at = 0;
    for (size_t r = 0; r + 1 < b.round_at.size(); ++r) {
        uint32_t rows_before = 0;   // of the round: where a staged segment's proofs start
        for (uint32_t s = b.round_at[r]; s < b.round_at[r + 1]; ++s) {
            const G16kSeg& S = b.segs[s];
            const G16kGroup& G = groups[S.group];
            const size_t in_bytes = (size_t)32 * G.K->n_inputs;
            hs[s].k = view[S.group];
            hs[s].inputs = staged ? b.din + S.in_at : G.inputs + in_bytes * S.first;
            hs[s].proofs = staged ? b.dpr + (size_t)387 * rows_before : G.proofs + (size_t)387 * S.first;
            hs[s].ok = G.ok + S.first;
            hs[s].count = S.rows;
            rows_before += S.rows;
            for (uint32_t q = 0; q < S.rows; q += G16K_BLOCK) hb[at++] = {s, q};
        }
    }
    BZK_HIP(ctx, hipMemcpyAsync(b.dsegs, hs, b.hsegs.size(), hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipMemcpyAsync(b.dblocks, hb, b.hblocks.size(), hipMemcpyHostToDevice, ctx->stream));
    const SegRec* dsegs = (const SegRec*)b.dsegs;
    uint32_t block0 = 0;
    for (size_t r = 0; r + 1 < b.round_at.size(); ++r) {
        if (staged)   // one stream: the round's rows follow the previous round's kernels into the staging buffers
            for (uint32_t s = b.round_at[r]; s < b.round_at[r + 1]; ++s) {
                const G16kSeg& S = b.segs[s];
                const G16kGroup& G = groups[S.group];
                const size_t in_bytes = (size_t)32 * G.K->n_inputs;
                if (in_bytes)
                    BZK_HIP(ctx, hipMemcpyAsync((void*)hs[s].inputs, G.inputs + in_bytes * S.first, in_bytes * S.rows, hipMemcpyHostToDevice, ctx->stream));
                BZK_HIP(ctx, hipMemcpyAsync((void*)hs[s].proofs, G.proofs + (size_t)387 * S.first, (size_t)387 * S.rows, hipMemcpyHostToDevice, ctx->stream));
            }
        const BlockRec* dblocks = (const BlockRec*)b.dblocks + block0;
        const dim3 grid(b.round_blocks[r]), block(G16K_BLOCK);
        BZK_LAUNCH(ctx, "g16k_prepare", g16k_prepare_kernel, grid, block, 0, dsegs, dblocks, b.slab, b.stride, b.sc, b.flags);
        BZK_LAUNCH(ctx, "g16k_miller", g16k_miller_kernel, grid, block, 0, dsegs, dblocks, b.slab, b.stride, b.flags);
        BZK_LAUNCH(ctx, "g16k_finalexp", g16k_finalexp_kernel, grid, block, 0, dsegs, dblocks, b.slab, b.stride, (const uint32_t*)b.flags);
        block0 += b.round_blocks[r];
    }
    if (sync) BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BZK_OK;
}

// the same per-proof functions on host threads over ALL rows of the groups in one task loop (host pointers; an invalid key gives zeros)
void g16k_host_run(const std::vector<G16kGroup>& groups) {
    std::vector<uint64_t> at(groups.size() + 1, 0);
    for (size_t g = 0; g < groups.size(); ++g) at[g + 1] = at[g] + groups[g].count;
    host_for_each(at.back(), host_default_threads(), [&](uint64_t i) {
        const size_t g = (size_t)(std::upper_bound(at.begin(), at.end(), i) - at.begin()) - 1;
        const G16kGroup& G = groups[g];
        const uint64_t j = i - at[g];
        host_one(*G.K, G.inputs + (size_t)32 * G.K->n_inputs * j, G.proofs + (size_t)387 * j, G.ok + j);
    });
}

}  // namespace bzk

using namespace bzk;

extern "C" {

int32_t bzk_groth16_verify_batch_keys(bzk_ctx* ctx, uint32_t n_keys, const uint8_t* vks, const uint64_t* vk_off, const uint32_t* n_inputs,
                                      const uint32_t* key_of, const uint8_t* inputs, const uint8_t* proofs, uint64_t n, uint8_t* ok) {
    if (n == 0) return BZK_OK;
    if (n_keys == 0 || !vks || !vk_off || !n_inputs || !key_of || !proofs || !ok) return BZK_E_ARG;
    if (!keys_well_formed(n_keys, vk_off)) return BZK_E_ARG;
    // a stable counting sort by key: row i is row pos[i] of the grouped order, group k the rows [first[k], first[k + 1]) of it
    std::vector<uint64_t> first(n_keys + 1, 0), pos(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (key_of[i] >= n_keys) return BZK_E_ARG;
        ++first[key_of[i] + 1];
    }
    std::vector<uint8_t> use(n_keys);
    size_t total_in = 0;
    for (uint32_t k = 0; k < n_keys; ++k) {
        use[k] = first[k + 1] != 0;
        total_in += (size_t)32 * n_inputs[k] * first[k + 1];
        first[k + 1] += first[k];
    }
    if (total_in && !inputs) return BZK_E_ARG;
    Keys K;
    prepare_keys(K, n_keys, vks, vk_off, n_inputs, use, ctx != nullptr);
    std::vector<size_t> in_at(n_keys + 1, 0);   // where a group's inputs start in the grouped order
    for (uint32_t k = 0; k < n_keys; ++k) in_at[k + 1] = in_at[k] + (size_t)32 * n_inputs[k] * (first[k + 1] - first[k]);
    {
        std::vector<uint64_t> next(first.begin(), first.end() - 1);
        for (uint64_t i = 0; i < n; ++i) pos[i] = next[key_of[i]]++;
    }
    if (!ctx) {   // every proof a task of one loop, in the caller's order
        std::vector<size_t> row_at(n);
        size_t at = 0;
        for (uint64_t i = 0; i < n; ++i) {
            row_at[i] = at;
            at += (size_t)32 * n_inputs[key_of[i]];
        }
        host_for_each(n, host_default_threads(), [&](uint64_t i) { host_one(K.key[key_of[i]], inputs + row_at[i], proofs + 387 * i, ok + i); });
        return BZK_OK;
    }
    (void)hipSetDevice(ctx->device);
    std::vector<uint8_t> gin(total_in + 1), gpr((size_t)387 * n), gok(n, 0);   // the grouped rows and their verdicts
    {
        size_t at = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t k = key_of[i];
            const size_t in_bytes = (size_t)32 * n_inputs[k];
            if (in_bytes) memcpy(gin.data() + in_at[k] + in_bytes * (pos[i] - first[k]), inputs + at, in_bytes);
            memcpy(gpr.data() + 387 * pos[i], proofs + 387 * i, 387);
            at += in_bytes;
        }
    }
    std::vector<G16kGroup> dev, wide;
    std::vector<uint32_t> dev_key;
    WsLayout ws("bzk_groth16_verify_batch_keys");
    G16kBufs b;
    uint8_t* dok = nullptr;
    for (uint32_t k = 0; k < n_keys; ++k) {
        if (!use[k] || !K.key[k].valid) continue;   // an invalid key: its rows of gok stay 0
        const uint64_t count = first[k + 1] - first[k];
        if (K.device(k)) {
            dev.push_back({&K.key[k], K.up[k].get(), count, gin.data() + in_at[k], gpr.data() + 387 * first[k], nullptr});
            dev_key.push_back(k);
        } else
            wide.push_back({&K.key[k], nullptr, count, gin.data() + in_at[k], gpr.data() + 387 * first[k], gok.data() + first[k]});
    }
    if (!dev.empty()) {
        g16k_declare(ws, b, dev, true);
        ws.take(dok, n);
        BZK_TRY(ws.commit(ctx));
        for (size_t g = 0; g < dev.size(); ++g) dev[g].ok = dok + first[dev_key[g]];
        BZK_TRY(g16k_enqueue(ctx, b, dev, true, false));
    }
    g16k_host_run(wide);   // beside the device's work
    for (size_t g = 0; g < dev.size(); ++g)
        BZK_HIP(ctx, hipMemcpyAsync(gok.data() + first[dev_key[g]], dev[g].ok, dev[g].count, hipMemcpyDeviceToHost, ctx->stream));
    if (!dev.empty()) BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the keys' upload buffers, the records and the layout go out of scope after this
    for (uint64_t i = 0; i < n; ++i) ok[i] = gok[pos[i]];
    return BZK_OK;
}

int32_t bzk_groth16_verify_groups_dev(bzk_ctx* ctx, uint32_t n_groups, const uint8_t* vks, const uint64_t* vk_off, const uint32_t* n_inputs,
                                      const uint64_t* counts, const void* inputs_dev, const void* proofs_dev, void* ok_dev) {
    if (!ctx) return BZK_E_ARG;
    if (n_groups == 0) return BZK_OK;
    if (!counts) return BZK_E_ARG;
    uint64_t n = 0;
    for (uint32_t g = 0; g < n_groups; ++g) n += counts[g];
    if (n == 0) return BZK_OK;
    if (!vks || !vk_off || !n_inputs || !proofs_dev || !ok_dev) return BZK_E_ARG;
    if (!keys_well_formed(n_groups, vk_off)) return BZK_E_ARG;
    std::vector<uint8_t> use(n_groups);
    std::vector<uint64_t> first(n_groups + 1, 0);
    std::vector<size_t> in_at(n_groups + 1, 0);
    for (uint32_t g = 0; g < n_groups; ++g) {
        use[g] = counts[g] != 0;
        first[g + 1] = first[g] + counts[g];
        in_at[g + 1] = in_at[g] + (size_t)32 * n_inputs[g] * counts[g];
    }
    if (in_at[n_groups] && !inputs_dev) return BZK_E_ARG;
    Keys K;
    prepare_keys(K, n_groups, vks, vk_off, n_inputs, use, true);
    (void)hipSetDevice(ctx->device);
    const uint8_t *din = (const uint8_t*)inputs_dev, *dpr = (const uint8_t*)proofs_dev;
    uint8_t* dok = (uint8_t*)ok_dev;
    std::vector<G16kGroup> dev, wide;
    std::vector<uint32_t> wide_group;
    size_t wide_in = 0, wide_n = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        if (!use[g]) continue;
        if (!K.key[g].valid)
            BZK_HIP(ctx, hipMemsetAsync(dok + first[g], 0, counts[g], ctx->stream));
        else if (K.device(g))
            dev.push_back({&K.key[g], K.up[g].get(), counts[g], din + in_at[g], dpr + 387 * first[g], dok + first[g]});
        else {
            wide.push_back({&K.key[g], nullptr, counts[g], nullptr, nullptr, nullptr});
            wide_group.push_back(g);
            wide_in += in_at[g + 1] - in_at[g];
            wide_n += counts[g];
        }
    }
    // the groups of more than 16 inputs: the host-thread path on copies, fetched before the device's work is queued and run beside it
    std::vector<uint8_t> hin(wide_in + 1), hpr((size_t)387 * wide_n + 1), hok(wide_n + 1);
    {
        size_t a_in = 0, a_n = 0;
        for (size_t w = 0; w < wide.size(); ++w) {
            const uint32_t g = wide_group[w];
            BZK_HIP(ctx, hipMemcpyAsync(hin.data() + a_in, din + in_at[g], in_at[g + 1] - in_at[g], hipMemcpyDeviceToHost, ctx->stream));
            BZK_HIP(ctx, hipMemcpyAsync(hpr.data() + 387 * a_n, dpr + 387 * first[g], (size_t)387 * counts[g], hipMemcpyDeviceToHost, ctx->stream));
            wide[w].inputs = hin.data() + a_in;
            wide[w].proofs = hpr.data() + 387 * a_n;
            wide[w].ok = hok.data() + a_n;
            a_in += in_at[g + 1] - in_at[g];
            a_n += counts[g];
        }
        if (!wide.empty()) BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    WsLayout ws("bzk_groth16_verify_groups_dev");
    G16kBufs b;
    if (!dev.empty()) {
        g16k_declare(ws, b, dev, false);
        BZK_TRY(ws.commit(ctx));
        BZK_TRY(g16k_enqueue(ctx, b, dev, false, false));
    }
    g16k_host_run(wide);
    for (size_t w = 0; w < wide.size(); ++w)
        BZK_HIP(ctx, hipMemcpyAsync(dok + first[wide_group[w]], wide[w].ok, wide[w].count, hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the keys' upload buffers, the records and the layout go out of scope after this
    return BZK_OK;
}

}  // extern "C"
