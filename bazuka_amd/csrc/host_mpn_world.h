// The MPN world behind the C ABI's opaque bzk_mpn handle: the sparse 4-ary account tree, the RAM state and the queues.  Shared by the prover
// (mpn.hip), which builds witnesses from it, and the wire-form admission entry points (wire.hip), which queue verified records into it.
#pragma once
#include <array>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "bzk_internal.h"
#include "host_mpn_types.h"  // Money, MpnAccount, MpnTx, {Update,Deposit,Withdraw}Transition

namespace bzk {

// ------------------------------------------------------------------------------------------------
// sparse 4-ary Poseidon tree
// ------------------------------------------------------------------------------------------------
struct SparseTree4 {
    int depth;
    std::vector<ZkScalar> defaults;                              // [0] = leaf default ... [depth] = empty root
    std::vector<std::unordered_map<uint64_t, ZkScalar>> level;   // level[0] = leaves
    SparseTree4(int d, const ZkScalar& leaf_default) : depth(d), level(d + 1) {
        defaults.push_back(leaf_default);
        for (int i = 0; i < d; ++i) {
            ZkScalar c[4] = {defaults.back(), defaults.back(), defaults.back(), defaults.back()};
            defaults.push_back(poseidon_hash(c, 4));
        }
    }
    ZkScalar get(int lv, uint64_t i) const {
        auto it = level[lv].find(i);
        return it == level[lv].end() ? defaults[lv] : it->second;
    }
    ZkScalar root() const { return get(depth, 0); }
    void set_leaf(uint64_t i, const ZkScalar& v) {
        level[0][i] = v;
        for (int lv = 0; lv < depth; ++lv) {
            const uint64_t base = i & ~(uint64_t)3;
            ZkScalar c[4] = {get(lv, base), get(lv, base + 1), get(lv, base + 2), get(lv, base + 3)};
            i >>= 2;
            level[lv + 1][i] = poseidon_hash(c, 4);
        }
    }
    // sibling triples, leaf level first (src/zk/state/mod.rs:218-264)
    std::vector<std::array<ZkScalar, 3>> prove(uint64_t i) const {
        std::vector<std::array<ZkScalar, 3>> out;
        for (int lv = 0; lv < depth; ++lv) {
            const uint64_t base = i & ~(uint64_t)3;
            std::array<ZkScalar, 3> t;
            int k = 0;
            for (uint64_t j = 0; j < 4; ++j)
                if (base + j != i) t[k++] = get(lv, base + j);
            out.push_back(t);
            i >>= 2;
        }
        return out;
    }
};

}  // namespace bzk

using namespace bzk;

// ------------------------------------------------------------------------------------------------
// the MPN world (RAM state) - opaque handle of the C ABI
// ------------------------------------------------------------------------------------------------
struct bzk_mpn {
    int L, T;
    ZkScalar token_default, tokens_tree_default, account_default;
    std::unique_ptr<SparseTree4> accounts, empty_tokens;
    std::map<uint64_t, MpnAccount> acct;
    std::map<uint64_t, JubjubPrivateKey> keys;
    std::vector<MpnTx> mempool;
    std::vector<DepositTx> deposit_queue;
    std::vector<WithdrawTx> withdraw_queue;
    uint64_t height = 0;
    ZkScalar contract_id = ZkScalar::from_u64(0x4D504E);  // ContractId::Custom of the MPN contract (payments of synthetic txs)
    int threads = host_default_threads();  // the CPUs this process may use (visible ones capped by the cgroup quota); bzk_mpn_set_threads overrides
    bzk_ctx* dev = nullptr;  // bzk_mpn_set_device: the witness builders hash their Merkle updates in batches on this context
    bool defer = false;      // bzk_mpn_set_defer: witness-only Update instances leave the hash-dependent values to the device (host_r1cs.h DeferProgram)
    bool defer_sig = false;  // bzk_mpn_set_defer_sig: ... and the signature gadget's ladders (implies `defer`)
    std::string dev_error;

    bzk_mpn(int l, int t) : L(l), T(t) {
        token_default = token_leaf(Money());
        empty_tokens.reset(new SparseTree4(T, token_default));
        tokens_tree_default = empty_tokens->root();
        account_default = account_hash(MpnAccount());
        accounts.reset(new SparseTree4(L, account_default));
    }
    SparseTree4 tokens_tree(const MpnAccount& a) const {
        SparseTree4 t = *empty_tokens;  // copy of the empty tree (defaults computed once)
        for (auto& kv : a.tokens) t.set_leaf(kv.first, token_leaf(kv.second));
        return t;
    }
    // the account tree's side of an account write whose token root the caller already has (`acct` is the caller's to write)
    void set_leaf_with_tokens_root(uint64_t i, const MpnAccount& a, const ZkScalar& tokens_root) {
        ZkScalar v[5] = {ZkScalar::from_u64(a.tx_nonce), ZkScalar::from_u64(a.withdraw_nonce), a.address.x, a.address.y, tokens_root};
        accounts->set_leaf(i, poseidon_hash(v, 5));
    }
    ZkScalar tokens_hash(const MpnAccount& a) const { return a.tokens.empty() ? tokens_tree_default : tokens_tree(a).root(); }
    ZkScalar account_hash(const MpnAccount& a) const {
        ZkScalar v[5] = {ZkScalar::from_u64(a.tx_nonce), ZkScalar::from_u64(a.withdraw_nonce), a.address.x, a.address.y, tokens_hash(a)};
        return poseidon_hash(v, 5);
    }
    MpnAccount get(uint64_t i) const {
        auto it = acct.find(i);
        return it == acct.end() ? MpnAccount() : it->second;
    }
    void set(uint64_t i, const MpnAccount& a) {
        acct[i] = a;
        accounts->set_leaf(i, account_hash(a));
    }
};

namespace bzk {
// what the last refused call of this thread said (bzk_mpn_work_last_error); defined in mpn.hip, set by the wire-form entry points too
extern thread_local std::string g_work_error;
}  // namespace bzk
