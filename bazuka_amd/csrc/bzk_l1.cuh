// Wire-form L1 transactions: the per-lane code of eddsa.hip's l1_tx_verify_kernel, l1_tx_hash_kernel and sha3_merkle_level_kernel, and what
// the parser (host_bincode.h parse_l1_txs) hands them.  __host__ __device__: the ctx = NULL entries and the kernels run the same functions.
//
//   Transaction::verify_signature   src/core/transaction.rs:386-397   Ed25519 over bincode(tx.sig_state_excluded())
//   Transaction::hash               :383-385                          SHA3-256 of the same bytes
//   MerkleTree::new / merge_hash    src/crypto/merkle.rs:9-19, 47-77, 93-108
//
// The signed bytes are hashed in place from the record as a gathered message (bzk_gather.cuh).
#pragma once
#include "bzk_ed25519.cuh"
#include "bzk_gather.cuh"
#include "bzk_keccak.cuh"
#include "bzk_l1.h"

namespace bzk {
namespace l1 {

// Transaction::verify_signature: src None verifies, Unsigned does not, else Ed25519 with R | A | signed form hashed in place
BZK_HD uint8_t verify_one(const uint8_t* data, const L1Rec& r, const uint32_t* __restrict__ base_tab, uint32_t* lane, int stride) {
    if (!(r.flags & HAS_SRC)) return 1;
    if (!(r.flags & SIGNED)) return 0;
    const gather::Msg m = gather::signed_form<true>(data, r.at, r.cut_a, r.cut_b, r.sig_tag, r.sig_off, r.key_off);
    return ed25519::verify_one(data + r.at + r.key_off, data + r.at + r.sig_off, m, base_tab, lane, stride);
}
// Transaction::hash
BZK_HD keccak::Digest hash_one(const uint8_t* data, const L1Rec& r) {
    return keccak::sha3_256_one(gather::signed_form<false>(data, r.at, r.cut_a, r.cut_b, r.sig_tag, 0, 0));
}

// ---- MerkleTree<Sha3Hasher>: n leaves make len = 2 n - 1 nodes in heap order (one zero node for n = 0)
struct TreeAt {
    uint32_t node_base;  // the tree's first node in the call's node array
    uint32_t len;        // its node count
};
BZK_HD uint32_t merkle_depth(uint32_t len) {  // len.next_power_of_two().trailing_zeros() - 1, 0 for len = 1
    uint32_t d = 0;
    while (d < 31 && ((uint32_t)1 << (d + 1)) < len) ++d;
    return d;
}
BZK_HD uint32_t merkle_leaf_map(uint32_t len, uint32_t i) {  // merkle.rs:47-59
    const uint32_t dep = merkle_depth(len), lower_start = ((uint32_t)1 << dep) - 1;
    if (lower_start + i < len) return lower_start + i;
    const uint32_t upper_start = ((uint32_t)1 << (dep - 1)) - 1;
    return upper_start - ((len - lower_start) >> 1) + i;
}
// the pairs make_parents merges at level d (1 .. depth): nodes 2^d - 1 + 2 k and the next, while inside the array
BZK_HD uint32_t merkle_level_pairs(uint32_t len, uint32_t d) {
    const uint32_t start = ((uint32_t)1 << d) - 1, stop = d >= 30 ? len : (((uint32_t)2 << d) - 1 < len ? ((uint32_t)2 << d) - 1 : len);
    return stop > start ? (stop - start) >> 1 : 0;
}
// merge_hash of pair k of level d into its parent; nodes: the tree's node array as words.  Smaller child first by byte-wise comparison.
BZK_HD void merkle_parent_one(uint32_t* nodes, uint32_t d, uint32_t k) {
    const uint32_t i = ((uint32_t)1 << d) - 1 + 2 * k;
    uint32_t a[8], b[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        a[w] = nodes[8 * (size_t)i + w];
        b[w] = nodes[8 * (size_t)(i + 1) + w];
    }
    bool less = false, decided = false;  // a < b as byte strings: the first differing word decides, read big-endian
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const uint32_t x = __builtin_bswap32(a[w]), y = __builtin_bswap32(b[w]);
        if (!decided && x != y) {
            less = x < y;
            decided = true;
        }
    }
    uint32_t lo[8], hi[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        lo[w] = less ? a[w] : b[w];
        hi[w] = less ? b[w] : a[w];
    }
    const keccak::Digest h = keccak::sha3_256_pair(lo, hi);
    uint32_t* out = nodes + 8 * (size_t)((i - 1) >> 1);
#pragma unroll
    for (int w = 0; w < 8; ++w) out[w] = h.w[w];
}
// the tree a lane belongs to: start has m + 1 non-decreasing entries, start[t] <= lane < start[t + 1]
BZK_HD uint32_t tree_of(const uint32_t* __restrict__ start, uint32_t m, uint32_t lane) {
    uint32_t lo = 0, hi = m;  // invariant: start[lo] <= lane < start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (start[mid] <= lane) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace l1
}  // namespace bzk
