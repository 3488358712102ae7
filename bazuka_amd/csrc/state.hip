// Row (b), seam "state compress": `ZkStateModel::compress<H>(&self, data: &ZkDataPairs) -> Result<ZkCompressedState, _>`
// (/root/reference/src/zk/mod.rs:392-399) for ANY state model - arbitrary nestings of Scalar / Struct{field_types} /
// List{log4_size, item_type} (src/zk/mod.rs:332-345) - over SPARSE (ZkDataLocator, ZkScalar) pairs.
//
// The reference builds a RAM KV store and replays `KvStoreStateManager::set_data` once per pair (src/zk/state/mod.rs:66-90, 310-420):
// depth-many hashes per pair, one at a time.  The value it ends with does not depend on the order of the pairs:
//   value(Scalar)  = the stored scalar, 0 when absent
//   value(Struct)  = H(value(field_0), ..., value(field_{k-1}))
//   value(List)    = root of the 4-ary tree over the 4^log4 items (node = H(c0, c1, c2, c3); log4 = 0: the item itself)
//   an untouched sub-tree has value compress_default(type) (src/zk/mod.rs:401-423)
//   state_size     = number of non-zero scalars stored (set_data's size_diff bookkeeping over an initially empty state)
// Here the touched part of that tree is laid out on the host (sorted locators -> nodes with their input lists, defaults as shared
// constants), nodes are grouped by (height, arity), and each group is ONE batched Poseidon launch on the device (K1): a node is hashed
// exactly once, level by level from the scalars up.  Dense shapes have dedicated, faster entries (bzk_merkle4_root: List{Scalar};
// bzk_mpn_state_compress_dev / bzk_mpn_tree_*: the MPN account model); this entry is the general seam.
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <unordered_map>

#include "bzk_internal.h"
#include "bzk_poseidon29_coop.cuh"
#include "bzk_state_chain.h"
#include "host_zk.h"

namespace bzk {
int32_t poseidon_launch(bzk_ctx* ctx, const void* in_dev, uint32_t arity, uint64_t n, void* out_dev);  // poseidon.hip
int32_t poseidon_consts_dev_shared(bzk_ctx* ctx, int t, const void** out, int* rf, int* rp);               // poseidon.hip
}

namespace {
using namespace bzk;

struct ModelNode {
    int kind = 0;  // 0 Scalar, 1 Struct, 2 List
    std::vector<int> fields;
    int log4 = 0, item = -1;
    ZkScalar dflt;                    // compress_default of this type
    std::vector<ZkScalar> list_dflt;  // List: default value of a node at depth k of its tree (k = log4: the item default, k = 0: = dflt)
};
struct Model {
    std::vector<ModelNode> nodes;
    int root = -1;
};

// bincode 1.3 (fixint, little endian): enum tag u32 - 0 Scalar, 1 Struct { field_types: Vec (u64 length) }, 2 List { log4_size: u8,
// item_type: Box } (declaration order of src/zk/mod.rs:332-345)
struct Rd {
    const uint8_t* p;
    uint64_t len, off = 0;
    bool ok = true;
    uint64_t u(int bytes) {
        if (!ok || off + bytes > len) { ok = false; return 0; }
        uint64_t v = 0;
        for (int i = 0; i < bytes; ++i) v |= (uint64_t)p[off + i] << (8 * i);
        off += bytes;
        return v;
    }
};
int parse_model(Rd& r, Model& M, int depth) {
    if (depth > 32 || M.nodes.size() > 100000) { r.ok = false; return -1; }
    const uint64_t tag = r.u(4);
    if (!r.ok) return -1;
    const int id = (int)M.nodes.size();
    M.nodes.emplace_back();
    if (tag == 0) {
        M.nodes[id].kind = 0;
    } else if (tag == 1) {
        M.nodes[id].kind = 1;
        const uint64_t k = r.u(8);
        // `is_valid`: at most MAX_ARITY fields (src/zk/mod.rs:355-367); an empty struct would hash zero values, for which no Poseidon
        // instance exists (the reference unwraps a missing parameter set)
        if (!r.ok || k == 0 || k > 16) { r.ok = false; return -1; }
        std::vector<int> f;
        for (uint64_t i = 0; i < k; ++i) {
            const int c = parse_model(r, M, depth + 1);
            if (c < 0) return -1;
            f.push_back(c);
        }
        M.nodes[id].fields = f;
    } else if (tag == 2) {
        M.nodes[id].kind = 2;
        const uint64_t lg = r.u(1);
        if (!r.ok || lg > 31) { r.ok = false; return -1; }  // indices are u64: 4^31 items at most
        const int c = parse_model(r, M, depth + 1);
        if (c < 0) return -1;
        M.nodes[id].log4 = (int)lg;
        M.nodes[id].item = c;
    } else {
        r.ok = false;
        return -1;
    }
    return id;
}
void model_defaults(Model& M, int id) {  // `compress_default` (src/zk/mod.rs:401-423), children first
    ModelNode& n = M.nodes[id];
    if (n.kind == 0) {
        n.dflt = ZkScalar::zero();
    } else if (n.kind == 1) {
        std::vector<ZkScalar> v;
        for (int f : n.fields) {
            model_defaults(M, f);
            v.push_back(M.nodes[f].dflt);
        }
        M.nodes[id].dflt = poseidon_hash(v);
    } else {
        model_defaults(M, n.item);
        ModelNode& nn = M.nodes[id];
        nn.list_dflt.assign((size_t)nn.log4 + 1, ZkScalar::zero());
        nn.list_dflt[nn.log4] = M.nodes[nn.item].dflt;
        for (int k = nn.log4 - 1; k >= 0; --k) {
            ZkScalar c[4] = {nn.list_dflt[k + 1], nn.list_dflt[k + 1], nn.list_dflt[k + 1], nn.list_dflt[k + 1]};
            nn.list_dflt[k] = poseidon_hash(c, 4);
        }
        nn.dflt = nn.list_dflt[0];
    }
}
int32_t load_model(const uint8_t* bytes, uint64_t len, Model& M) {
    if (!bytes) return BZK_E_ARG;
    Rd r{bytes, len};
    M.root = parse_model(r, M, 0);
    if (!r.ok || M.root < 0 || r.off != len) return BZK_E_ARG;
    model_defaults(M, M.root);
    return BZK_OK;
}

// the touched part of the state as a hash schedule
struct Plan {
    // value ids: [0, consts.size()) shared default constants, then the n pair values, then the hashed nodes
    std::vector<ZkScalar> consts;
    std::map<std::pair<int, int>, uint32_t> const_id;  // (model node, tree depth or -1) -> id
    struct Node { uint32_t first_in, arity, level; };
    std::vector<Node> nodes;      // hashed nodes in creation order
    std::vector<uint32_t> inputs;  // their input ids, back to back (node ids are offset by `hash_base` once all leaves are known)
    uint64_t n_pairs = 0;
    std::string err;
    int32_t code = 0;  // BZK_REFUSE_* of `err`
};
constexpr uint32_t HASHED = 0x80000000u;  // input id tag: index into Plan::nodes (resolved after levelling)

struct Builder {
    const Model& M;
    Plan& P;
    const uint64_t* loc_off;
    const uint64_t* loc;
    const std::vector<uint64_t>& order;  // pair indices, sorted by locator
    uint32_t cst(int model, int depth, const ZkScalar& v) {
        auto key = std::make_pair(model, depth);
        auto it = P.const_id.find(key);
        if (it != P.const_id.end()) return it->second;
        const uint32_t id = (uint32_t)P.consts.size();
        P.consts.push_back(v);
        P.const_id[key] = id;
        return id;
    }
    uint64_t at(uint64_t pos, uint64_t d) const { return loc[loc_off[order[pos]] + d]; }
    uint64_t len(uint64_t pos) const { return loc_off[order[pos] + 1] - loc_off[order[pos]]; }
    uint32_t level_of(uint32_t id) const { return (id & HASHED) ? P.nodes[id & ~HASHED].level : 0; }
    uint32_t hashed(const std::vector<uint32_t>& in) {
        uint32_t lv = 0;
        for (uint32_t x : in) lv = std::max(lv, level_of(x));
        if (P.nodes.size() >= 0x7ffffff0u) { P.err = "too many nodes"; P.code = BZK_REFUSE_OTHER; return 0; }
        P.nodes.push_back({(uint32_t)P.inputs.size(), (uint32_t)in.size(), lv + 1});
        P.inputs.insert(P.inputs.end(), in.begin(), in.end());
        return HASHED | (uint32_t)(P.nodes.size() - 1);
    }
    // value id of the sub-state of type `m` under the common prefix of length d shared by the sorted pairs [lo, hi) (non-empty)
    uint32_t build(int m, uint64_t d, uint64_t lo, uint64_t hi) {
        const ModelNode& n = M.nodes[m];
        if (!P.err.empty()) return 0;
        if (n.kind == 0) {
            // `set_data`: the locator must end exactly here (NonScalarLocatorError / LocatorError otherwise); a HashMap holds a key once
            if (hi - lo != 1) { P.err = "duplicate locator"; P.code = BZK_REFUSE_DUPLICATE_LOCATOR; return 0; }
            if (len(lo) != d) { P.err = "locator points below a scalar (ZkLocatorError::InvalidLocator)"; P.code = BZK_REFUSE_INVALID_LOCATOR; return 0; }
            return 0x40000000u | (uint32_t)order[lo];  // pair value, resolved to consts.size() + pair index
        }
        for (uint64_t i = lo; i < hi; ++i)
            if (len(i) <= d) { P.err = "locator does not reach a scalar (StateManagerError::NonScalarLocatorError)"; P.code = BZK_REFUSE_NON_SCALAR_LOCATOR; return 0; }
        if (n.kind == 1) {
            std::vector<uint32_t> in(n.fields.size());
            uint64_t i = lo;
            for (size_t f = 0; f < n.fields.size(); ++f) {
                uint64_t j = i;
                while (j < hi && at(j, d) == f) ++j;
                in[f] = j > i ? build(n.fields[f], d + 1, i, j) : cst(n.fields[f], -1, M.nodes[n.fields[f]].dflt);
                i = j;
            }
            if (i != hi) { P.err = "struct field index out of range (the reference indexes field_types out of bounds)"; P.code = BZK_REFUSE_INVALID_LOCATOR; return 0; }
            return hashed(in);
        }
        // List: items first, then the sparse 4-ary tree over them, level by level
        const uint64_t size = n.log4 >= 32 ? ~0ull : ((uint64_t)1 << (2 * n.log4));
        std::vector<std::pair<uint64_t, uint32_t>> cur;  // (index at the current depth, value id), ascending
        for (uint64_t i = lo; i < hi;) {
            const uint64_t idx = at(i, d);
            if (idx >= size) { P.err = "list index out of range (ZkLocatorError::InvalidLocator)"; P.code = BZK_REFUSE_INVALID_LOCATOR; return 0; }
            uint64_t j = i;
            while (j < hi && at(j, d) == idx) ++j;
            cur.push_back({idx, build(n.item, d + 1, i, j)});
            if (!P.err.empty()) return 0;
            i = j;
        }
        for (int k = n.log4; k > 0; --k) {  // children at depth k -> parents at depth k - 1
            const uint32_t dk = cst(m, k, n.list_dflt[k]);
            std::vector<std::pair<uint64_t, uint32_t>> up;
            for (size_t i = 0; i < cur.size();) {
                const uint64_t parent = cur[i].first >> 2;
                std::vector<uint32_t> in(4, dk);
                while (i < cur.size() && (cur[i].first >> 2) == parent) {
                    in[cur[i].first & 3] = cur[i].second;
                    ++i;
                }
                up.push_back({parent, hashed(in)});
            }
            cur.swap(up);
        }
        return cur[0].second;
    }
};

__global__ void __launch_bounds__(256) state_gather_kernel(const Fr* __restrict__ vals, const uint32_t* __restrict__ idx, uint64_t count,
                                                           Fr* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = vals[idx[i]];
}

int32_t compress_core(bzk_ctx* ctx, const Model& M, const uint64_t* loc_off, const uint64_t* loc, const uint8_t* values, uint64_t n,
                      uint8_t state_hash[32], uint64_t* state_size) {
    const ModelNode& root = M.nodes[M.root];
    uint64_t nz = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* v = values + 32 * i;
        bool any = false;
        for (int b = 0; b < 32; ++b) any |= v[b] != 0;
        nz += any;
        // Montgomery limbs of a residue: < r as an integer (a `ZkScalar` cannot hold anything else)
        Fr f;
        memcpy(f.l, v, 32);
        Fr g = f;
        fe_reduce_once<FrParams>(g);
        if (!g.equals(f)) { ctx->last_error = "state_compress: a value is not a canonical field element"; ctx->last_refusal = BZK_REFUSE_NON_CANONICAL_VALUE; return BZK_E_ARG; }
    }
    if (state_size) *state_size = nz;
    if (n == 0) {
        root.dflt.to_bytes(state_hash);
        return BZK_OK;
    }
    if (n >= 0x3fffffffull) return BZK_E_ARG;
    // sort the pairs by locator (lexicographic; a proper prefix sorts first and is then reported as an error by the builder)
    std::vector<uint64_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    for (uint64_t i = 0; i < n; ++i)
        if (loc_off[i] > loc_off[i + 1]) return BZK_E_ARG;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        return std::lexicographical_compare(loc + loc_off[a], loc + loc_off[a + 1], loc + loc_off[b], loc + loc_off[b + 1]);
    });
    Plan P;
    P.n_pairs = n;
    Builder B{M, P, loc_off, loc, order};
    const uint32_t top = B.build(M.root, 0, 0, n);
    if (!P.err.empty()) {
        ctx->last_error = "state_compress: " + P.err;
        ctx->last_refusal = P.code;
        return BZK_E_ARG;
    }
    const uint32_t n_const = (uint32_t)P.consts.size();
    const uint32_t hash_base = n_const + (uint32_t)n;
    if (!(top & HASHED)) {  // the model is a bare Scalar (or a chain of log4 = 0 lists down to one): the value itself
        memcpy(state_hash, values + 32 * (size_t)(top & 0x3fffffffu), 32);
        return BZK_OK;
    }
    // group the hashed nodes by (level, arity): final id = hash_base + rank in that order
    const size_t nn = P.nodes.size();
    std::vector<uint32_t> by(nn), rank(nn);
    std::iota(by.begin(), by.end(), 0u);
    std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) {
        if (P.nodes[a].level != P.nodes[b].level) return P.nodes[a].level < P.nodes[b].level;
        return P.nodes[a].arity < P.nodes[b].arity;
    });
    for (size_t r = 0; r < nn; ++r) rank[by[r]] = (uint32_t)r;
    auto resolve = [&](uint32_t id) -> uint32_t {
        if (id & HASHED) return hash_base + rank[id & ~HASHED];
        if (id & 0x40000000u) return n_const + (id & 0x3fffffffu);
        return id;
    };
    std::vector<uint32_t> gidx;  // gather indices of all groups, back to back in group order
    gidx.reserve(P.inputs.size());
    struct Group { uint32_t arity; uint64_t count, in_off, first_rank; };
    std::vector<Group> groups;
    for (size_t r = 0; r < nn;) {
        const Plan::Node& a = P.nodes[by[r]];
        size_t e = r;
        while (e < nn && P.nodes[by[e]].level == a.level && P.nodes[by[e]].arity == a.arity) ++e;
        groups.push_back({a.arity, (uint64_t)(e - r), (uint64_t)gidx.size(), (uint64_t)r});
        for (size_t q = r; q < e; ++q) {
            const Plan::Node& x = P.nodes[by[q]];
            for (uint32_t k = 0; k < x.arity; ++k) gidx.push_back(resolve(P.inputs[x.first_in + k]));
        }
        r = e;
    }
    // device: values array (constants | pair values | hashed nodes), gather indices, one staging buffer for the widest group
    uint64_t widest = 0;
    for (auto& g : groups) widest = std::max<uint64_t>(widest, g.count * g.arity);
    (void)hipSetDevice(ctx->device);
    WsLayout ws("compress_core");
    Fr *d_vals, *d_in;
    uint32_t* d_idx;
    ws.take(d_vals, (size_t)hash_base + nn); ws.take(d_idx, gidx.size()); ws.take(d_in, widest);
    BZK_TRY(ws.commit(ctx));
    BZK_HIP(ctx, hipMemcpyAsync(d_vals, P.consts.data(), (size_t)n_const * 32, hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipMemcpyAsync(d_vals + n_const, values, (size_t)n * 32, hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipMemcpyAsync(d_idx, gidx.data(), gidx.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    for (auto& g : groups) {
        const uint64_t cnt = g.count * g.arity;
        BZK_LAUNCH(ctx, "state_gather", state_gather_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (const Fr*)d_vals,
                   (const uint32_t*)(d_idx + g.in_off), cnt, d_in);
        BZK_TRY(poseidon_launch(ctx, d_in, g.arity, g.count, d_vals + hash_base + g.first_rank));
    }
    BZK_TRY(pinned_reserve(ctx, 64));
    BZK_HIP(ctx, hipMemcpyAsync(ctx->pinned, d_vals + resolve(top), 32, hipMemcpyDeviceToHost, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // also: the host vectors above outlive every copy out of them
    memcpy(state_hash, ctx->pinned, 32);
    return BZK_OK;
}


// ------------------------------------------------------------------------------------------------------------------------------
// PERSISTENT device state of one contract, any model: `KvStoreStateManager::{update_contract, set_data, get_data, prove, root}`
// (/root/reference/src/zk/state/mod.rs:218-438) with the VALUES resident in HBM.
//
// The reference keeps every scalar and every non-default node in a KV store and walks root-wards once per written scalar
// (depth-many hashes, one at a time, each sibling a KV read).  Here the store is one device array of 32-byte slots: [0, n_const)
// the defaults of the model (compress_default per type and per tree depth), then one slot per scalar / struct / list / inner tree
// node that was ever touched.  The host keeps only the INDEX (key -> slot) and one bit per scalar (zero / non-zero, for
// state_size).  One `update_contract` = one plan: the union of the root-ward paths of all written scalars, every node once,
// grouped by (height, arity) -> one gather + one batched Poseidon launch (K1) + one scatter per group, in place.  Untouched
// siblings are read from their slots on the device; nothing but the new scalars goes up and nothing but the root comes back.
//   key of a value at a locator            = the locator
//   key of an inner node of a list's tree  = locator of the list ++ {AUX | depth, index at that depth}   (0 < depth < log4_size)
// Nodes that return to their default stay in the index (the reference removes them): same values either way.
// ------------------------------------------------------------------------------------------------------------------------------
using sc::AUX;
using sc::Key;
using sc::KeyHash;

__global__ void __launch_bounds__(256) state_scatter_kernel(const Fr* __restrict__ in, const uint32_t* __restrict__ dst, uint64_t count,
                                                            Fr* __restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) vals[dst[i]] = in[i];
}

// ---- the chain's kernels (bzk_state_update_chain): a level of every (node, time) pair of a round in ONE launch - the inputs fetched through source
// indices (bzk_state_chain.h: top bit = the round's arena, else the value store), the hash written to the node's arena position.  The store and the
// arena are two buffers and the output IS the arena: no __restrict__ between them.  What makes a launch safe is the plan - a group only reads versions
// of lower levels.  Widths 2 .. 8 (poseidon29_hash / poseidon29_coop_val); wider structs run as gather, poseidon_launch.
__device__ __forceinline__ Fr chain_load(const Fr* vals, const Fr* arena, uint32_t s) {
    return (s & sc::SRC_ARENA) ? arena[s & ~sc::SRC_ARENA] : vals[s];
}
// one lane per node
template <int T>
__global__ void __launch_bounds__(128) state_chain_hash_kernel(const Fr* vals, Fr* arena, const uint32_t* __restrict__ src, uint64_t n, uint64_t first,
                                                               const Fr29* __restrict__ consts, int rf, int rp) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr in[T - 1];
#pragma unroll
    for (int k = 0; k < T - 1; ++k) in[k] = chain_load(vals, arena, src[i * (T - 1) + k]);
    arena[first + i] = poseidon29_hash<T>(in, consts, rf, rp);
}
// eight lanes per node (lane j of a group fetches input j - 1), for groups too small to fill the machine: poseidon_launch's reasoning and its bound
template <int T>
__global__ void __launch_bounds__(64) state_chain_hash_coop_kernel(const Fr* vals, Fr* arena, const uint32_t* __restrict__ src, uint64_t n, uint64_t first,
                                                                   const Fr29* __restrict__ consts, int rf, int rp) {
    const uint64_t node = (uint64_t)blockIdx.x * 8 + (threadIdx.x >> 3);
    const uint64_t p = node < n ? node : n - 1;  // whole groups stay convergent for the shuffles
    const int j = threadIdx.x & 7, jj = j < T ? j : T - 1;
    const Fr mine = chain_load(vals, arena, src[p * (T - 1) + (jj >= 1 ? jj - 1 : 0)]);
    const Fr h = poseidon29_coop_val<T>(mine, consts, rf, rp);
    if (node < n && j == 1) arena[first + p] = h;
}
typedef void (*chain_hash_fn)(const Fr*, Fr*, const uint32_t*, uint64_t, uint64_t, const Fr29*, int, int);
chain_hash_fn chain_hash_table(int t, bool coop) {
    switch (t) {
        case 2: return coop ? state_chain_hash_coop_kernel<2> : state_chain_hash_kernel<2>;
        case 3: return coop ? state_chain_hash_coop_kernel<3> : state_chain_hash_kernel<3>;
        case 4: return coop ? state_chain_hash_coop_kernel<4> : state_chain_hash_kernel<4>;
        case 5: return coop ? state_chain_hash_coop_kernel<5> : state_chain_hash_kernel<5>;
        case 6: return coop ? state_chain_hash_coop_kernel<6> : state_chain_hash_kernel<6>;
        case 7: return coop ? state_chain_hash_coop_kernel<7> : state_chain_hash_kernel<7>;
        case 8: return coop ? state_chain_hash_coop_kernel<8> : state_chain_hash_kernel<8>;
        default: return nullptr;
    }
}
constexpr uint64_t CHAIN_COOP_MAX_NODES = 8192;  // poseidon.hip COOP_MAX_NODES
// the inputs of a wide group, side by side for poseidon_launch
__global__ void __launch_bounds__(256) state_chain_gather_kernel(const Fr* vals, const Fr* arena, const uint32_t* __restrict__ src, uint64_t count,
                                                                 Fr* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = chain_load(vals, arena, src[i]);
}
// the commit of a prefix: the host has de-duplicated `dst`, no two lanes write one slot
__global__ void __launch_bounds__(256) state_chain_commit_kernel(const Fr* __restrict__ arena, const uint32_t* __restrict__ from, const uint32_t* __restrict__ dst,
                                                                 uint64_t count, Fr* __restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) vals[dst[i]] = arena[from[i]];
}

}  // namespace

struct bzk_state {
    bzk_ctx* ctx = nullptr;
    int device = 0;
    Model M;
    std::vector<uint32_t> dflt_slot;                // per model node: slot of compress_default(type)
    std::vector<std::vector<uint32_t>> depth_slot;  // lists: slot of the default of a node at depth k of the tree (k = 0 .. log4)
    uint32_t n_const = 0;
    Fr* d_vals = nullptr;
    size_t cap = 0, used = 0;
    std::unordered_map<Key, uint32_t, KeyHash> slot_of;
    std::vector<uint8_t> nonzero;  // per slot; meaningful for scalar slots
    uint64_t size = 0, height = 0;
    uint8_t root_hash[32];
    bool poisoned = false;  // a device error in the middle of an update: the slots no longer describe one state
    std::mutex m;
    const uint32_t* find_slot(const Key& k) const {  // what sc::Updater reads the index through
        auto it = slot_of.find(k);
        return it != slot_of.end() ? &it->second : nullptr;
    }
    // every call that used the store has synchronised its stream before returning, and the context is not touched here: a host that
    // tears its handles down in arbitrary order (a garbage collector) may already have destroyed it
    ~bzk_state() {
        if (d_vals) {
            (void)hipSetDevice(device);
            (void)hipFree(d_vals);
        }
    }
};

namespace {

int32_t state_grow(bzk_state* S, size_t need) {
    if (need <= S->cap) return BZK_OK;
    bzk_ctx* ctx = S->ctx;
    size_t cap = std::max<size_t>(S->cap * 2, 4096);
    while (cap < need) cap *= 2;
    if (cap >= 0x7fffffffull) cap = 0x7fffffffull;
    if (need > cap) { ctx->last_error = "state: more than 2^31 slots"; return BZK_E_ALLOC; }
    Fr* nv = nullptr;
    if (hipMalloc(&nv, cap * sizeof(Fr)) != hipSuccess) {
        (void)hipGetLastError();
        ctx->last_error = "state: out of device memory growing the value store";
        return BZK_E_ALLOC;
    }
    if (S->used) {
        hipError_t e = hipMemcpyAsync(nv, S->d_vals, S->used * sizeof(Fr), hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(nv);
            ctx->last_error = std::string("state: copying the value store: ") + hipGetErrorString(e);
            return BZK_E_DEVICE;
        }
    }
    if (S->d_vals) (void)hipFree(S->d_vals);
    S->d_vals = nv;
    S->cap = cap;
    return BZK_OK;
}

// `ZkStateModel::locate` (src/zk/mod.rs:367-390): the model node a locator names, -1 where the reference errors (or indexes
// field_types out of bounds)
int state_locate(const Model& M, const uint64_t* loc, uint64_t len) {
    int m = M.root;
    for (uint64_t i = 0; i < len; ++i) {
        const ModelNode& n = M.nodes[m];
        if (n.kind == 1) {
            if (loc[i] >= n.fields.size()) return -1;
            m = n.fields[loc[i]];
        } else if (n.kind == 2) {
            if (n.log4 < 32 && loc[i] >= ((uint64_t)1 << (2 * n.log4))) return -1;
            m = n.item;
        } else {
            return -1;
        }
    }
    return m;
}

// gathers `idx.size()` slots and brings them to the host
int32_t state_read_slots(bzk_state* S, const std::vector<uint32_t>& idx, uint8_t* out) {
    bzk_ctx* ctx = S->ctx;
    if (idx.empty()) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    WsLayout ws("state_read_slots");
    uint32_t* d_idx;
    Fr* d_out;
    ws.take(d_idx, idx.size()); ws.take(d_out, idx.size());
    BZK_TRY(ws.commit(ctx));
    BZK_HIP(ctx, hipMemcpyAsync(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    BZK_LAUNCH(ctx, "state_gather", state_gather_kernel, dim3((unsigned)((idx.size() + 255) / 256)), dim3(256), 0, (const Fr*)S->d_vals,
               (const uint32_t*)d_idx, (uint64_t)idx.size(), d_out);
    BZK_HIP(ctx, hipMemcpyAsync(out, d_out, idx.size() * 32, hipMemcpyDeviceToHost, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BZK_OK;
}

// the plan of one update_contract and the walk that makes it: bzk_state_chain.h (shared with the chain planner)
using sc::UpPlan;
typedef sc::Updater<bzk_state> Updater;

int32_t state_update_impl(bzk_state* S, const uint64_t* loc_off, const uint64_t* loc, const uint8_t* values, uint64_t n, uint64_t target_height,
                          uint8_t* prev_values_out) {
    bzk_ctx* ctx = S->ctx;
    if (S->poisoned) { ctx->last_error = "state: an earlier update failed on the device; this state is unusable"; return BZK_E_DEVICE; }
    if (n >= 0x3fffffffull) return BZK_E_ARG;
    for (uint64_t i = 0; i < n; ++i) {
        if (loc_off[i] > loc_off[i + 1]) return BZK_E_ARG;
        Fr f;
        memcpy(f.l, values + 32 * i, 32);
        Fr g = f;
        fe_reduce_once<FrParams>(g);
        if (!g.equals(f)) { ctx->last_error = "state_update: a value is not a canonical field element"; ctx->last_refusal = BZK_REFUSE_NON_CANONICAL_VALUE; return BZK_E_ARG; }
    }
    if (n == 0) {
        S->height = target_height;
        return BZK_OK;
    }
    std::vector<uint64_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        return std::lexicographical_compare(loc + loc_off[a], loc + loc_off[a + 1], loc + loc_off[b], loc + loc_off[b + 1]);
    });
    UpPlan P;
    P.next_slot = (uint32_t)S->used;
    P.scalar_dst.assign(n, 0);
    Updater U{*S, P, loc_off, loc, order, {}};
    const Updater::Val top = U.build(S->M.root, 0, 0, n);
    if (!P.err.empty()) {
        ctx->last_error = "state_update: " + P.err;
        ctx->last_refusal = P.code;
        return BZK_E_ARG;
    }
    (void)hipSetDevice(ctx->device);
    BZK_TRY(state_grow(S, P.next_slot));
    // the rollback of this delta (`ZkState::push_delta`, src/zk/mod.rs:521-530): what the named scalars held before; 0 = nothing
    if (prev_values_out) {
        std::vector<uint32_t> idx;
        std::vector<uint64_t> which;
        for (uint64_t i = 0; i < n; ++i) {
            if (P.scalar_dst[i] < S->used) {
                idx.push_back(P.scalar_dst[i]);
                which.push_back(i);
            } else {
                memset(prev_values_out + 32 * i, 0, 32);
            }
        }
        std::vector<uint8_t> got(idx.size() * 32);
        BZK_TRY(state_read_slots(S, idx, got.data()));
        for (size_t q = 0; q < which.size(); ++q) memcpy(prev_values_out + 32 * which[q], got.data() + 32 * q, 32);
    }
    // groups of equal (level, arity), lowest level first
    const size_t nn = P.nodes.size();
    std::vector<uint32_t> by(nn);
    std::iota(by.begin(), by.end(), 0u);
    std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t b) {
        if (P.nodes[a].level != P.nodes[b].level) return P.nodes[a].level < P.nodes[b].level;
        return P.nodes[a].arity < P.nodes[b].arity;
    });
    struct Group { uint32_t arity; uint64_t count, in_off, dst_off; };
    std::vector<Group> groups;
    std::vector<uint32_t> gidx, gdst;
    gidx.reserve(P.inputs.size());
    gdst.reserve(nn);
    uint64_t widest = n;
    for (size_t r = 0; r < nn;) {
        const UpPlan::Node& a = P.nodes[by[r]];
        size_t e = r;
        while (e < nn && P.nodes[by[e]].level == a.level && P.nodes[by[e]].arity == a.arity) ++e;
        groups.push_back({a.arity, (uint64_t)(e - r), (uint64_t)gidx.size(), (uint64_t)gdst.size()});
        for (size_t q = r; q < e; ++q) {
            const UpPlan::Node& x = P.nodes[by[q]];
            for (uint32_t k = 0; k < x.arity; ++k) gidx.push_back(P.inputs[x.first_in + k]);
            gdst.push_back(x.dst);
        }
        widest = std::max<uint64_t>(widest, (uint64_t)(e - r) * a.arity);
        r = e;
    }
    WsLayout ws("state_update_impl");
    Fr *d_new, *d_in, *d_out;
    uint32_t *d_sdst, *d_idx, *d_dst;
    ws.take(d_new, n); ws.take(d_sdst, n); ws.take(d_idx, gidx.size()); ws.take(d_dst, gdst.size());
    ws.take(d_in, widest); ws.take(d_out, widest);
    BZK_TRY(ws.commit(ctx));
    // the sources of these copies are pageable vectors of this frame and the caller's `values`: no early return may leave one of
    // them in flight - a failed upload waits for the stream before it reports
    auto upload = [&]() -> int32_t {
        BZK_HIP(ctx, hipMemcpyAsync(d_new, values, (size_t)n * 32, hipMemcpyHostToDevice, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(d_sdst, P.scalar_dst.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!gidx.empty()) BZK_HIP(ctx, hipMemcpyAsync(d_idx, gidx.data(), gidx.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        if (!gdst.empty()) BZK_HIP(ctx, hipMemcpyAsync(d_dst, gdst.data(), gdst.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        return BZK_OK;
    };
    if (const int32_t up = upload(); up != BZK_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        return up;  // no slot was written yet: the state is still the old one
    }
    // from here on the slots change: a failure leaves them half-written
    auto run = [&]() -> int32_t {
        BZK_LAUNCH(ctx, "state_scatter", state_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const Fr*)d_new, (const uint32_t*)d_sdst,
                   n, S->d_vals);
        for (auto& g : groups) {
            const uint64_t cnt = g.count * g.arity;
            BZK_LAUNCH(ctx, "state_gather", state_gather_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (const Fr*)S->d_vals,
                       (const uint32_t*)(d_idx + g.in_off), cnt, d_in);
            BZK_TRY(poseidon_launch(ctx, d_in, g.arity, g.count, d_out));
            BZK_LAUNCH(ctx, "state_scatter", state_scatter_kernel, dim3((unsigned)((g.count + 255) / 256)), dim3(256), 0, (const Fr*)d_out,
                       (const uint32_t*)(d_dst + g.dst_off), g.count, S->d_vals);
        }
        BZK_TRY(pinned_reserve(ctx, 64));
        BZK_HIP(ctx, hipMemcpyAsync(ctx->pinned, S->d_vals + top.slot, 32, hipMemcpyDeviceToHost, ctx->stream));
        BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return BZK_OK;
    };
    const int32_t st = run();
    if (st != BZK_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // whatever was queued reads this frame's vectors: let it finish (or fail) first
        S->poisoned = true;
        return st;
    }
    memcpy(S->root_hash, ctx->pinned, 32);
    S->used = P.next_slot;
    S->nonzero.resize(S->used, 0);
    for (auto& nk : P.new_keys) S->slot_of.emplace(std::move(nk.first), nk.second);
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* v = values + 32 * i;
        bool now = false;
        for (int b = 0; b < 32; ++b) now |= v[b] != 0;
        uint8_t& was = S->nonzero[P.scalar_dst[i]];
        if (now && !was) ++S->size;
        if (!now && was) --S->size;
        was = now ? 1 : 0;
    }
    S->height = target_height;
    return BZK_OK;
}

// ---- bzk_state_update_chain: m deltas through the tree together (bzk_state_chain.h).  m_out >= m verdicts are written; tail_refusal (or NULL): delta m
// exists but did not decode - it is refused for that reason if the deltas before it all apply
int32_t state_chain_impl(bzk_state* S, uint64_t m, uint64_t m_out, const char* tail_refusal, const uint64_t* delta_off, const uint64_t* loc_off,
                         const uint64_t* loc, const uint8_t* values, const uint64_t* heights, const uint8_t* claims, uint64_t round_versions,
                         uint8_t* states_out, uint8_t* verdict, uint64_t* applied, uint8_t* prev_out) {
    bzk_ctx* ctx = S->ctx;
    if (S->poisoned) { ctx->last_error = "state: an earlier update failed on the device; this state is unusable"; return BZK_E_DEVICE; }
    for (uint64_t j = 0; j < m; ++j)
        if (delta_off[j] > delta_off[j + 1]) return BZK_E_ARG;
    const uint64_t pairs = m ? delta_off[m] : 0;
    for (uint64_t i = m ? delta_off[0] : 0; i < pairs; ++i)
        if (loc_off[i] > loc_off[i + 1]) return BZK_E_ARG;
    memset(states_out, 0, (size_t)m_out * 40);
    memset(verdict, BZK_CHAIN_NOT_REACHED, (size_t)m_out);
    *applied = 0;
    if (prev_out && pairs) memset(prev_out, 0, (size_t)pairs * 32);
    sc::ChainPlanner<bzk_state> PL(*S);
    PL.plan(m, delta_off, loc_off, loc, values, [](const uint8_t* v) {
        Fr f;
        memcpy(f.l, v, 32);
        Fr g = f;
        fe_reduce_once<FrParams>(g);
        return g.equals(f);
    });
    const uint64_t mp = PL.deltas.size();
    (void)hipSetDevice(ctx->device);
    // the rollbacks that only the store knows: scalars the call's first writer of a slot finds there.  Read before anything is committed
    std::vector<uint8_t> resident;
    std::vector<uint64_t> resident_at(PL.prev_of.size(), 0);
    if (prev_out) {
        std::vector<uint32_t> idx;
        uint64_t q = 0;
        for (uint64_t j = 0; j < mp; ++j)
            for (uint64_t i = 0; i < PL.deltas[j].n; ++i, ++q)
                if (PL.prev_of[q] == sc::PREV_RESIDENT) {
                    resident_at[q] = idx.size();
                    idx.push_back(PL.deltas[j].P.scalar_dst[i]);
                }
        resident.resize(idx.size() * 32);
        BZK_TRY(state_read_slots(S, idx, resident.data()));
    }
    const std::vector<uint64_t> cuts = PL.rounds(round_versions);
    std::vector<sc::ChainRound> R(cuts.size() - 1);
    uint64_t cap_v = 0, cap_src = 0, cap_in = 0, cap_d = 0, cap_w = 0;
    for (size_t r = 0; r < R.size(); ++r) {
        R[r].resolve(PL.deltas, cuts[r], cuts[r + 1]);
        cap_v = std::max(cap_v, R[r].n_versions);
        cap_src = std::max<uint64_t>(cap_src, R[r].src.size());
        cap_in = std::max(cap_in, R[r].widest_in);
        cap_d = std::max(cap_d, R[r].d1 - R[r].d0);
        cap_w = std::max<uint64_t>(cap_w, R[r].writes.size());
    }
    WsLayout ws("state_chain_impl");
    Fr *d_arena, *d_in, *d_roots;
    uint32_t *d_src, *d_rix, *d_from, *d_dst;
    ws.take(d_arena, cap_v); ws.take(d_src, cap_src); ws.take(d_in, cap_in); ws.take(d_rix, cap_d); ws.take(d_roots, cap_d);
    ws.take(d_from, cap_w); ws.take(d_dst, cap_w);
    if (mp) BZK_TRY(ws.commit(ctx));
    uint64_t done = 0;  // deltas that are part of the state now
    bool stopped = false;
    std::vector<uint32_t> rix, from, dst;
    std::vector<uint8_t> roots;
    for (size_t r = 0; r < R.size() && !stopped; ++r) {
        const sc::ChainRound& C = R[r];
        // every index a lane will follow, checked here: a plain source is a slot of the store as it stands, an arena source a version of this round
        for (uint32_t s : C.src)
            if ((s & sc::SRC_ARENA) ? (s & ~sc::SRC_ARENA) >= C.n_versions : s >= S->used) { ctx->last_error = "state_update_chain: a source index out of range"; return BZK_E_INTERNAL; }
        rix.clear();
        for (uint32_t x : C.root_ix)
            if (x != sc::NO_ROOT) {
                if (x >= C.n_versions) { ctx->last_error = "state_update_chain: a root index out of range"; return BZK_E_INTERNAL; }
                rix.push_back(x);
            }
        roots.assign(rix.size() * 32, 0);
        // pageable sources (the caller's values, this frame's vectors): whatever was queued finishes before an error returns
        auto run = [&]() -> int32_t {
            if (C.n_up) BZK_HIP(ctx, hipMemcpyAsync(d_arena, values + 32 * C.pair0, (size_t)C.n_up * 32, hipMemcpyHostToDevice, ctx->stream));
            if (!C.src.empty()) BZK_HIP(ctx, hipMemcpyAsync(d_src, C.src.data(), C.src.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            for (const sc::ChainRound::Group& g : C.groups) {
                const int t = (int)g.arity + 1;
                if (t <= 8) {
                    const void* consts;
                    int rf, rp;
                    BZK_TRY(poseidon_consts_dev_shared(ctx, t, &consts, &rf, &rp));
                    if (g.count <= CHAIN_COOP_MAX_NODES && !ctx->no_coop) {
                        BZK_LAUNCH(ctx, "state_chain_hash_coop", chain_hash_table(t, true), dim3((unsigned)((g.count + 7) / 8)), dim3(64), 0, (const Fr*)S->d_vals,
                                   d_arena, (const uint32_t*)(d_src + g.src_off), g.count, g.first, (const Fr29*)consts, rf, rp);
                    } else {
                        const uint64_t blocks = (g.count + 127) / 128;
                        if (blocks > 0x7fffffffull) return BZK_E_ARG;
                        BZK_LAUNCH(ctx, "state_chain_hash", chain_hash_table(t, false), dim3((unsigned)blocks), dim3(128), 0, (const Fr*)S->d_vals, d_arena,
                                   (const uint32_t*)(d_src + g.src_off), g.count, g.first, (const Fr29*)consts, rf, rp);
                    }
                } else {
                    const uint64_t cnt = g.count * g.arity;
                    BZK_LAUNCH(ctx, "state_chain_gather", state_chain_gather_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (const Fr*)S->d_vals,
                               (const Fr*)d_arena, (const uint32_t*)(d_src + g.src_off), cnt, d_in);
                    BZK_TRY(poseidon_launch(ctx, d_in, g.arity, g.count, d_arena + g.first));
                }
            }
            if (!rix.empty()) {
                BZK_HIP(ctx, hipMemcpyAsync(d_rix, rix.data(), rix.size() * 4, hipMemcpyHostToDevice, ctx->stream));
                BZK_LAUNCH(ctx, "state_gather", state_gather_kernel, dim3((unsigned)((rix.size() + 255) / 256)), dim3(256), 0, (const Fr*)d_arena,
                           (const uint32_t*)d_rix, (uint64_t)rix.size(), d_roots);
                BZK_HIP(ctx, hipMemcpyAsync(roots.data(), d_roots, rix.size() * 32, hipMemcpyDeviceToHost, ctx->stream));
            }
            BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            return BZK_OK;
        };
        if (const int32_t st = run(); st != BZK_OK) {
            (void)hipStreamSynchronize(ctx->stream);
            if (st == BZK_E_DEVICE) S->poisoned = true;
            return st;
        }
        // the states of the round and the prefix of it that holds
        std::vector<uint8_t> states((size_t)(C.d1 - C.d0) * 40);
        uint8_t cur[32];
        memcpy(cur, S->root_hash, 32);
        uint64_t upto = C.d1, q = 0;
        for (uint64_t j = C.d0; j < C.d1; ++j) {
            if (C.root_ix[j - C.d0] != sc::NO_ROOT) memcpy(cur, roots.data() + 32 * q++, 32);
            uint8_t* s40 = states.data() + 40 * (j - C.d0);
            memcpy(s40, cur, 32);
            memcpy(s40 + 32, &PL.deltas[j].size_after, 8);
            if (upto == C.d1 && claims && memcmp(s40, claims + 40 * j, 40) != 0) upto = j;
        }
        if (upto > C.d0) {
            BZK_TRY(state_grow(S, PL.deltas[upto - 1].used_after));
            C.commit_lists(upto, from, dst);
            auto commit = [&]() -> int32_t {
                if (dst.empty()) return BZK_OK;
                BZK_HIP(ctx, hipMemcpyAsync(d_from, from.data(), from.size() * 4, hipMemcpyHostToDevice, ctx->stream));
                BZK_HIP(ctx, hipMemcpyAsync(d_dst, dst.data(), dst.size() * 4, hipMemcpyHostToDevice, ctx->stream));
                BZK_LAUNCH(ctx, "state_chain_commit", state_chain_commit_kernel, dim3((unsigned)((dst.size() + 255) / 256)), dim3(256), 0, (const Fr*)d_arena,
                           (const uint32_t*)d_from, (const uint32_t*)d_dst, (uint64_t)dst.size(), S->d_vals);
                BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
                return BZK_OK;
            };
            for (size_t i = 0; i < dst.size(); ++i)
                if (dst[i] >= S->cap || from[i] >= C.n_versions) { ctx->last_error = "state_update_chain: a commit index out of range"; return BZK_E_INTERNAL; }
            if (const int32_t st = commit(); st != BZK_OK) {
                (void)hipStreamSynchronize(ctx->stream);
                S->poisoned = true;  // the slots may be half-written
                return st;
            }
            sc::commit_index(*S, PL.deltas, C.d0, upto, values);
            memcpy(S->root_hash, states.data() + 40 * (upto - 1 - C.d0), 32);
            S->height = heights[upto - 1];
            done = upto;
        }
        const uint64_t shown = upto < C.d1 ? upto + 1 : upto;  // a mismatching delta shows the state it gives
        memcpy(states_out + 40 * C.d0, states.data(), (size_t)(shown - C.d0) * 40);
        memset(verdict + C.d0, BZK_CHAIN_APPLIED, (size_t)(upto - C.d0));
        if (upto < C.d1) {
            verdict[upto] = BZK_CHAIN_MISMATCH;
            stopped = true;
        }
    }
    *applied = done;
    if (!stopped && (PL.refused || (tail_refusal && mp == m))) {
        verdict[mp] = BZK_CHAIN_REFUSED;
        ctx->last_error = "state_update_chain: delta " + std::to_string(mp) + ": " + (PL.refused ? PL.refuse_err : std::string(tail_refusal));
        ctx->last_refusal = PL.refused ? PL.refuse_code : BZK_REFUSE_OTHER;
    }
    if (prev_out) {
        uint64_t q = 0;
        for (uint64_t j = 0; j < mp; ++j)
            for (uint64_t i = 0; i < PL.deltas[j].n; ++i, ++q) {
                if (j >= done) continue;
                const int64_t from_pair = PL.prev_of[q];
                if (from_pair >= 0) memcpy(prev_out + 32 * (PL.deltas[j].pair0 + i), values + 32 * from_pair, 32);
                else if (from_pair == sc::PREV_RESIDENT) memcpy(prev_out + 32 * (PL.deltas[j].pair0 + i), resident.data() + 32 * resident_at[q], 32);
            }
    }
    return BZK_OK;
}

}  // namespace

namespace bzk {
int32_t hash_plan_run(bzk_ctx* ctx, const uint8_t* uploaded, uint64_t n_up, const std::vector<HashGroup>& groups, std::vector<uint8_t>& hashed_out) {
    if (!ctx || (n_up && !uploaded)) return BZK_E_ARG;
    uint64_t n_hash = 0, n_idx = 0, widest = 0;
    for (auto& g : groups) {
        if (g.arity < 1 || g.arity > 16 || g.in.size() % g.arity) return BZK_E_ARG;
        for (uint32_t id : g.in)
            if (id >= n_up + n_hash) return BZK_E_INTERNAL;  // a group may only consume earlier values
        n_hash += g.count();
        n_idx += g.in.size();
        widest = std::max<uint64_t>(widest, g.in.size());
    }
    hashed_out.assign((size_t)n_hash * 32, 0);
    if (!n_hash) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    WsLayout ws("hash_plan_run");
    Fr *d_vals, *d_in;
    uint32_t* d_idx;
    ws.take(d_vals, n_up + n_hash); ws.take(d_idx, n_idx); ws.take(d_in, widest);
    BZK_TRY(ws.commit(ctx));
    std::vector<uint32_t> all;
    all.reserve(n_idx);
    for (auto& g : groups) all.insert(all.end(), g.in.begin(), g.in.end());
    if (n_up) BZK_HIP(ctx, hipMemcpyAsync(d_vals, uploaded, (size_t)n_up * 32, hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipMemcpyAsync(d_idx, all.data(), all.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    uint64_t off = 0, out = n_up;
    for (auto& g : groups) {
        const uint64_t cnt = g.in.size();
        if (!cnt) continue;
        BZK_LAUNCH(ctx, "state_gather", state_gather_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, (const Fr*)d_vals,
                   (const uint32_t*)(d_idx + off), cnt, d_in);
        BZK_TRY(poseidon_launch(ctx, d_in, g.arity, g.count(), d_vals + out));
        off += cnt;
        out += g.count();
    }
    BZK_HIP(ctx, hipMemcpyAsync(hashed_out.data(), d_vals + n_up, (size_t)n_hash * 32, hipMemcpyDeviceToHost, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return BZK_OK;
}
}  // namespace bzk

// bzk_last_refusal (include/bzk.h): every public state call starts with "not refused"; a BZK_E_ARG that no site classified is OTHER
template <class Fn>
static int32_t refusal_scope(bzk_ctx* ctx, Fn&& fn) {
    if (ctx) ctx->last_refusal = BZK_REFUSE_NONE;
    const int32_t st = fn();
    if (ctx) {
        if (st != BZK_E_ARG) ctx->last_refusal = BZK_REFUSE_NONE;
        else if (ctx->last_refusal == BZK_REFUSE_NONE) ctx->last_refusal = BZK_REFUSE_OTHER;
    }
    return st;
}

extern "C" {

int32_t bzk_state_model_default(const uint8_t* model, uint64_t model_len, uint8_t out[32]) {
    if (!out) return BZK_E_ARG;
    Model M;
    BZK_TRY(load_model(model, model_len, M));
    M.nodes[M.root].dflt.to_bytes(out);
    return BZK_OK;
}

static int32_t state_entry_compress(bzk_ctx* ctx, const uint8_t* model, uint64_t model_len, const uint64_t* loc_off, const uint64_t* loc,
                           const uint8_t* values, uint64_t n, uint8_t state_hash[32], uint64_t* state_size) {
    if (!ctx || !state_hash || (n && (!loc_off || !values))) return BZK_E_ARG;
    if (n && loc_off[n] && !loc) return BZK_E_ARG;
    Model M;
    if (load_model(model, model_len, M) != BZK_OK) {
        ctx->last_error = "state_compress: not a bincode ZkStateModel (or a struct with 0 / more than 16 fields)";
        return BZK_E_ARG;
    }
    static const uint64_t zero_off[1] = {0};
    return compress_core(ctx, M, n ? loc_off : zero_off, loc, values, n, state_hash, state_size);
}

// pairs = bincode(ZkDataPairs) = HashMap<ZkDataLocator, ZkScalar>: u64 count, then per entry Vec<u64> (u64 length + items) and the
// scalar's four Montgomery limbs (src/zk/mod.rs:202-206, 425-426, 469-470).  out = bincode(ZkCompressedState) = state_hash | u64 state_size
static int32_t state_entry_compress_bincode(bzk_ctx* ctx, const uint8_t* model, uint64_t model_len, const uint8_t* pairs, uint64_t pairs_len,
                                   uint8_t compressed_out[40]) {
    if (!ctx || !pairs || !compressed_out) return BZK_E_ARG;
    Rd r{pairs, pairs_len};
    const uint64_t n = r.u(8);
    if (!r.ok || n > pairs_len / 40) return BZK_E_ARG;
    std::vector<uint64_t> off(1, 0), loc;
    std::vector<uint8_t> vals;
    vals.reserve((size_t)n * 32);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t k = r.u(8);
        if (!r.ok || k > 64) return BZK_E_ARG;
        for (uint64_t j = 0; j < k; ++j) loc.push_back(r.u(8));
        off.push_back(loc.size());
        if (!r.ok || r.off + 32 > pairs_len) return BZK_E_ARG;
        vals.insert(vals.end(), pairs + r.off, pairs + r.off + 32);
        r.off += 32;
    }
    if (!r.ok || r.off != pairs_len) return BZK_E_ARG;
    uint64_t size = 0;
    BZK_TRY(state_entry_compress(ctx, model, model_len, off.data(), loc.data(), vals.data(), n, compressed_out, &size));
    memcpy(compressed_out + 32, &size, 8);
    return BZK_OK;
}

int32_t bzk_state_create(bzk_ctx* ctx, const uint8_t* model, uint64_t model_len, bzk_state** out) {
    if (!ctx || !out) return BZK_E_ARG;
    *out = nullptr;
    std::unique_ptr<bzk_state> S(new (std::nothrow) bzk_state);
    if (!S) return BZK_E_ALLOC;
    S->ctx = ctx;
    S->device = ctx->device;
    if (load_model(model, model_len, S->M) != BZK_OK) {
        ctx->last_error = "state_create: not a bincode ZkStateModel (or a struct with 0 / more than 16 fields)";
        return BZK_E_ARG;
    }
    std::vector<ZkScalar> consts;
    S->dflt_slot.assign(S->M.nodes.size(), 0);
    S->depth_slot.assign(S->M.nodes.size(), {});
    for (size_t i = 0; i < S->M.nodes.size(); ++i) {
        const ModelNode& n = S->M.nodes[i];
        S->dflt_slot[i] = (uint32_t)consts.size();
        consts.push_back(n.dflt);
        if (n.kind == 2) {
            for (int k = 0; k <= n.log4; ++k) {
                S->depth_slot[i].push_back((uint32_t)consts.size());
                consts.push_back(n.list_dflt[k]);
            }
        }
    }
    S->n_const = (uint32_t)consts.size();
    (void)hipSetDevice(ctx->device);
    BZK_TRY(state_grow(S.get(), S->n_const));
    std::vector<uint8_t> bytes(consts.size() * 32);
    for (size_t i = 0; i < consts.size(); ++i) consts[i].to_bytes(bytes.data() + 32 * i);
    BZK_HIP(ctx, hipMemcpyAsync(S->d_vals, bytes.data(), bytes.size(), hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    S->used = S->n_const;
    S->nonzero.assign(S->used, 0);
    S->M.nodes[S->M.root].dflt.to_bytes(S->root_hash);
    *out = S.release();
    return BZK_OK;
}

void bzk_state_free(bzk_state* st) {
    delete st;  // frees the value store (see ~bzk_state)
}

static int32_t state_entry_update(bzk_state* st, const uint64_t* loc_off, const uint64_t* loc, const uint8_t* values, uint64_t n, uint64_t target_height,
                         uint8_t state_hash[32], uint64_t* state_size, uint8_t* prev_values_out) {
    if (!st || (n && (!loc_off || !values))) return BZK_E_ARG;
    if (n && loc_off[n] && !loc) return BZK_E_ARG;
    std::lock_guard<std::mutex> g(st->m);
    static const uint64_t zero_off[1] = {0};
    BZK_TRY(state_update_impl(st, n ? loc_off : zero_off, loc, values, n, target_height, prev_values_out));
    if (state_hash) memcpy(state_hash, st->root_hash, 32);
    if (state_size) *state_size = st->size;
    return BZK_OK;
}

// delta = bincode(ZkDeltaPairs) = HashMap<ZkDataLocator, Option<ZkScalar>> (src/zk/mod.rs:473-474): u64 count; per entry Vec<u64>,
// the Option's u8 tag, the four Montgomery limbs when Some.  None writes zero, as `update_contract` does (`v.unwrap_or_default()`).
// One decoder for bzk_state_update_bincode and for every blob of bzk_state_update_chain_bincode.
// appends the pairs of one blob: their locators to (off, loc), their values (zeros for None) to vals; false when the bytes are not one ZkDeltaPairs
static bool delta_decode_append(const uint8_t* delta, uint64_t delta_len, std::vector<uint64_t>& off, std::vector<uint64_t>& loc, std::vector<uint8_t>& vals,
                                uint64_t* n_out) {
    Rd r{delta, delta_len};
    const uint64_t n = r.u(8);
    if (!r.ok || n > delta_len / 9) return false;
    const size_t v0 = vals.size();
    vals.resize(v0 + (size_t)n * 32, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t k = r.u(8);
        if (!r.ok || k > 64) return false;
        for (uint64_t j = 0; j < k; ++j) loc.push_back(r.u(8));
        off.push_back(loc.size());
        const uint64_t tag = r.u(1);
        if (!r.ok || tag > 1) return false;
        if (tag) {
            if (r.off + 32 > delta_len) return false;
            memcpy(vals.data() + v0 + 32 * i, delta + r.off, 32);
            r.off += 32;
        }
    }
    if (!r.ok || r.off != delta_len) return false;
    *n_out = n;
    return true;
}
static int32_t state_entry_update_bincode(bzk_state* st, const uint8_t* delta, uint64_t delta_len, uint64_t target_height, uint8_t compressed_out[40]) {
    if (!st || !delta || !compressed_out) return BZK_E_ARG;
    std::vector<uint64_t> off(1, 0), loc;
    std::vector<uint8_t> vals;
    uint64_t n = 0;
    if (!delta_decode_append(delta, delta_len, off, loc, vals, &n)) return BZK_E_ARG;
    uint64_t size = 0;
    BZK_TRY(state_entry_update(st, off.data(), loc.data(), vals.data(), n, target_height, compressed_out, &size, nullptr));
    memcpy(compressed_out + 32, &size, 8);
    return BZK_OK;
}

// a refused delta of a chain is a verdict under BZK_OK: the refusal outlives the call's status, unlike refusal_scope's
static int32_t state_entry_update_chain(bzk_state* st, uint64_t m, uint64_t m_out, const char* tail_refusal, const uint64_t* delta_off, const uint64_t* loc_off,
                                        const uint64_t* loc, const uint8_t* values, const uint64_t* target_heights, const uint8_t* claims, uint64_t round_versions,
                                        uint8_t* states_out, uint8_t* verdict, uint64_t* applied, uint8_t* prev_values_out) {
    std::lock_guard<std::mutex> g(st->m);
    st->ctx->last_refusal = BZK_REFUSE_NONE;
    const int32_t s = state_chain_impl(st, m, m_out, tail_refusal, delta_off, loc_off, loc, values, target_heights, claims, round_versions, states_out, verdict,
                                       applied, prev_values_out);
    if (s == BZK_E_ARG) st->ctx->last_refusal = BZK_REFUSE_OTHER;
    return s;
}
int32_t bzk_state_update_chain(bzk_state* st, uint64_t m, const uint64_t* delta_off, const uint64_t* loc_off, const uint64_t* loc, const uint8_t* values,
                               const uint64_t* target_heights, const uint8_t* claims, uint64_t round_versions, uint8_t* states_out, uint8_t* verdict,
                               uint64_t* applied, uint8_t* prev_values_out) {
    if (!st) return BZK_E_ARG;
    if (m == 0) {  // a no-op that refuses nothing
        st->ctx->last_refusal = BZK_REFUSE_NONE;
        if (applied) *applied = 0;
        return BZK_OK;
    }
    if (!delta_off || !target_heights || !states_out || !verdict || !applied) return BZK_E_ARG;
    if (delta_off[m] && (!loc_off || !values)) return BZK_E_ARG;
    if (delta_off[m] && delta_off[0] <= delta_off[m] && loc_off[delta_off[m]] && !loc) return BZK_E_ARG;
    static const uint64_t zero_off[1] = {0};
    return state_entry_update_chain(st, m, m, nullptr, delta_off, delta_off[m] ? loc_off : zero_off, loc, values, target_heights, claims, round_versions, states_out,
                                    verdict, applied, prev_values_out);
}
int32_t bzk_state_update_chain_bincode(bzk_state* st, uint64_t m, const uint8_t* deltas, const uint64_t* delta_byte_off, const uint64_t* target_heights,
                                       const uint8_t* claims, uint64_t round_versions, uint8_t* states_out, uint8_t* verdict, uint64_t* applied) {
    if (!st) return BZK_E_ARG;
    if (m == 0) {  // a no-op that refuses nothing
        st->ctx->last_refusal = BZK_REFUSE_NONE;
        if (applied) *applied = 0;
        return BZK_OK;
    }
    if (!deltas || !delta_byte_off || !target_heights || !states_out || !verdict || !applied) return BZK_E_ARG;
    for (uint64_t j = 0; j < m; ++j)
        if (delta_byte_off[j] > delta_byte_off[j + 1]) return BZK_E_ARG;
    std::vector<uint64_t> d_off(1, 0), off(1, 0), loc;
    std::vector<uint8_t> vals;
    uint64_t good = 0;  // the blobs before the first that does not decode
    for (; good < m; ++good) {
        const size_t o0 = off.size(), l0 = loc.size(), v0 = vals.size();
        uint64_t n = 0;
        if (!delta_decode_append(deltas + delta_byte_off[good], delta_byte_off[good + 1] - delta_byte_off[good], off, loc, vals, &n)) {
            off.resize(o0), loc.resize(l0), vals.resize(v0);
            break;
        }
        d_off.push_back(d_off.back() + n);
    }
    if (loc.empty()) loc.push_back(0);
    if (vals.empty()) vals.resize(32, 0);
    return state_entry_update_chain(st, good, m, good < m ? "not a bincode ZkDeltaPairs" : nullptr, d_off.data(), off.data(), loc.data(), vals.data(), target_heights,
                                    claims, round_versions, states_out, verdict, applied, nullptr);
}

int32_t bzk_state_root(bzk_state* st, uint8_t state_hash[32], uint64_t* state_size, uint64_t* height) {
    if (!st) return BZK_E_ARG;
    std::lock_guard<std::mutex> g(st->m);
    if (st->poisoned) return BZK_E_DEVICE;
    if (state_hash) memcpy(state_hash, st->root_hash, 32);
    if (state_size) *state_size = st->size;
    if (height) *height = st->height;
    return BZK_OK;
}

// `get_data` for n locators: the value at each (a scalar, or the hash of the struct / list it names), the type's default where
// nothing was ever written
static int32_t state_entry_get(bzk_state* st, const uint64_t* loc_off, const uint64_t* loc, uint64_t n, uint8_t* values_out) {
    if (!st || (n && (!loc_off || !values_out))) return BZK_E_ARG;
    if (n && loc_off[n] && !loc) return BZK_E_ARG;
    std::lock_guard<std::mutex> g(st->m);
    if (st->poisoned) return BZK_E_DEVICE;
    if (n >= 0x3fffffffull) return BZK_E_ARG;
    std::vector<uint32_t> idx(n);
    Key k;
    for (uint64_t i = 0; i < n; ++i) {
        if (loc_off[i] > loc_off[i + 1]) return BZK_E_ARG;
        const uint64_t* l = loc + loc_off[i];
        const uint64_t len = loc_off[i + 1] - loc_off[i];
        const int m = state_locate(st->M, l, len);
        if (m < 0) {
            st->ctx->last_error = "state_get: the locator names nothing in this model (ZkLocatorError::InvalidLocator)";
            st->ctx->last_refusal = BZK_REFUSE_INVALID_LOCATOR;
            return BZK_E_ARG;
        }
        k.assign(l, l + len);
        auto it = st->slot_of.find(k);
        idx[i] = it != st->slot_of.end() ? it->second : st->dflt_slot[m];
    }
    return state_read_slots(st, idx, values_out);
}

// `prove` (src/zk/state/mod.rs:218-264) for n indices of the list at `tree_loc`: per index log4_size x 3 scalars, leaf level first,
// the three siblings of each level in ascending position
static int32_t state_entry_prove(bzk_state* st, const uint64_t* tree_loc, uint64_t tree_loc_len, const uint64_t* indices, uint64_t n, uint8_t* proof_out,
                        uint32_t* log4_size) {
    if (!st || (tree_loc_len && !tree_loc) || (n && (!indices || !proof_out))) return BZK_E_ARG;
    std::lock_guard<std::mutex> g(st->m);
    if (st->poisoned) return BZK_E_DEVICE;
    const int m = state_locate(st->M, tree_loc, tree_loc_len);
    if (m < 0) {
        st->ctx->last_error = "state_prove: the locator names nothing in this model (ZkLocatorError::InvalidLocator)";
        st->ctx->last_refusal = BZK_REFUSE_INVALID_LOCATOR;
        return BZK_E_ARG;
    }
    const ModelNode& nd = st->M.nodes[m];
    if (nd.kind != 2) {
        st->ctx->last_error = "state_prove: not locating a tree (StateManagerError::NonTreeLocatorError)";
        st->ctx->last_refusal = BZK_REFUSE_NON_TREE_LOCATOR;
        return BZK_E_ARG;
    }
    if (log4_size) *log4_size = (uint32_t)nd.log4;
    if ((uint64_t)nd.log4 * 3 * n >= 0x3fffffffull) return BZK_E_ARG;
    std::vector<uint32_t> idx;
    idx.reserve((size_t)n * nd.log4 * 3);
    Key k(tree_loc, tree_loc + tree_loc_len);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t cur = indices[i];
        if (nd.log4 < 32 && cur >= ((uint64_t)1 << (2 * nd.log4))) {
            st->ctx->last_error = "state_prove: index beyond the list";
            st->ctx->last_refusal = BZK_REFUSE_INVALID_LOCATOR;
            return BZK_E_ARG;
        }
        for (int d = nd.log4; d > 0; --d) {  // siblings at depth d
            const uint64_t first = cur & ~(uint64_t)3;
            for (uint64_t j = first; j < first + 4; ++j) {
                if (j == cur) continue;
                if (d == nd.log4) {
                    k.push_back(j);
                } else {
                    k.push_back(AUX | (uint64_t)d);
                    k.push_back(j);
                }
                auto it = st->slot_of.find(k);
                idx.push_back(it != st->slot_of.end() ? it->second : st->depth_slot[m][d]);
                k.resize(tree_loc_len);
            }
            cur >>= 2;
        }
    }
    return state_read_slots(st, idx, proof_out);
}

int32_t bzk_state_stats(bzk_state* st, uint64_t* slots, uint64_t* device_bytes, uint64_t* keys) {
    if (!st) return BZK_E_ARG;
    std::lock_guard<std::mutex> g(st->m);
    if (slots) *slots = st->used;
    if (device_bytes) *device_bytes = st->cap * sizeof(Fr);
    if (keys) *keys = st->slot_of.size();
    return BZK_OK;
}

int32_t bzk_state_compress(bzk_ctx* ctx, const uint8_t* model, uint64_t model_len, const uint64_t* loc_off, const uint64_t* loc, const uint8_t* values, uint64_t n, uint8_t state_hash[32], uint64_t* state_size) {
    return refusal_scope(ctx, [&] { return state_entry_compress(ctx, model, model_len, loc_off, loc, values, n, state_hash, state_size); });
}
int32_t bzk_state_compress_bincode(bzk_ctx* ctx, const uint8_t* model, uint64_t model_len, const uint8_t* pairs, uint64_t pairs_len, uint8_t compressed_out[40]) {
    return refusal_scope(ctx, [&] { return state_entry_compress_bincode(ctx, model, model_len, pairs, pairs_len, compressed_out); });
}
int32_t bzk_state_update(bzk_state* st, const uint64_t* loc_off, const uint64_t* loc, const uint8_t* values, uint64_t n, uint64_t target_height, uint8_t state_hash[32], uint64_t* state_size, uint8_t* prev_values_out) {
    return refusal_scope((st ? st->ctx : nullptr), [&] { return state_entry_update(st, loc_off, loc, values, n, target_height, state_hash, state_size, prev_values_out); });
}
int32_t bzk_state_update_bincode(bzk_state* st, const uint8_t* delta, uint64_t delta_len, uint64_t target_height, uint8_t compressed_out[40]) {
    return refusal_scope((st ? st->ctx : nullptr), [&] { return state_entry_update_bincode(st, delta, delta_len, target_height, compressed_out); });
}
int32_t bzk_state_get(bzk_state* st, const uint64_t* loc_off, const uint64_t* loc, uint64_t n, uint8_t* values_out) {
    return refusal_scope((st ? st->ctx : nullptr), [&] { return state_entry_get(st, loc_off, loc, n, values_out); });
}
int32_t bzk_state_prove(bzk_state* st, const uint64_t* tree_loc, uint64_t tree_loc_len, const uint64_t* indices, uint64_t n, uint8_t* proof_out, uint32_t* log4_size) {
    return refusal_scope((st ? st->ctx : nullptr), [&] { return state_entry_prove(st, tree_loc, tree_loc_len, indices, n, proof_out, log4_size); });
}

}  // extern "C"
