// The host side of the persistent device state (state.hip): the walk that turns one delta into a hash plan (Updater), and the planner that
// sends a CHAIN of deltas through the tree together (bzk_state_update_chain).  Plain C++, no HIP calls: tests/host/state_chain_check.hip drives
// it against a value store in host memory.
//
// Every template here reads its state through the same few members, which bzk_state (state.hip) and the check's host state both have:
//   M.nodes[i].{kind, fields, log4, item}, M.root   the model (0 Scalar, 1 Struct, 2 List)
//   dflt_slot, depth_slot                           slots of the defaults per model node / per depth of a list's tree
//   slot_of                                         key -> slot (std::unordered_map<Key, uint32_t, KeyHash>)
//   used, nonzero, size                             slots handed out, zero / non-zero per scalar slot, number of non-zero scalars
//
// A chain of m deltas.  The levels of the tree do not depend on time: a node after delta j needs its children as they stood after delta j.  So every
// written scalar and every hashed node of delta j becomes a VERSION, all versions of a round live in one arena (the uploaded scalars at its front,
// in pair order; the hashed nodes behind them, grouped by (level, arity)), and a group is one launch over every (node, time) pair of its level.
// An input of a hash is a SOURCE INDEX, resolved here: the latest version of its slot so far in the round - top bit set, the low 31 bits index
// the arena - else the resident slot (slots stay below 2^31), else the default slot the walk chose.  level(version) = 1 + the largest level of
// its inputs, resident slots and uploaded scalars being level 0: no group reads what it writes.  Nothing in the value store changes until the
// roots are back and compared: then the prefix that holds is committed, one write per slot from its latest version inside the prefix.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <numeric>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/bzk.h"
#include "bzk_rounds.h"

namespace bzk {
namespace sc {

constexpr uint64_t AUX = (uint64_t)1 << 63;  // no list index reaches it: 4^31 items at most
typedef std::vector<uint64_t> Key;
struct KeyHash {
    size_t operator()(const Key& k) const {
        uint64_t h = 0x9e3779b97f4a7c15ull ^ k.size();
        for (uint64_t x : k) {
            h ^= x + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
            h *= 0xff51afd7ed558ccdull;
            h ^= h >> 33;
        }
        return (size_t)h;
    }
};
typedef std::unordered_map<Key, uint32_t, KeyHash> KeyIndex;

// the plan of one update_contract
struct UpPlan {
    struct Node { uint32_t dst, first_in, arity, level; };
    std::vector<Node> nodes;
    std::vector<uint32_t> inputs;                    // slots
    std::vector<std::pair<Key, uint32_t>> new_keys;  // index entries to add once the update has run
    std::vector<uint32_t> scalar_dst;                // per pair: its slot
    uint32_t next_slot = 0;
    std::string err;
    int32_t code = 0;  // BZK_REFUSE_* of `err`
};
// St: the members listed at the top, or an Overlay of them (find_slot)
template <class St>
struct Updater {
    St& S;
    UpPlan& P;
    const uint64_t* loc_off;
    const uint64_t* loc;
    const std::vector<uint64_t>& order;
    Key prefix;
    struct Val { uint32_t slot, level; };
    uint64_t at(uint64_t pos, uint64_t d) const { return loc[loc_off[order[pos]] + d]; }
    uint64_t len(uint64_t pos) const { return loc_off[order[pos] + 1] - loc_off[order[pos]]; }
    uint32_t slot_for(const Key& k) {  // the slot of a key that is being written: its own, or a fresh one
        if (const uint32_t* s = S.find_slot(k)) return *s;
        if (P.next_slot >= 0x7ffffff0u) { P.err = "too many nodes"; P.code = BZK_REFUSE_OTHER; return 0; }
        P.new_keys.push_back({k, P.next_slot});
        return P.next_slot++;
    }
    uint32_t read_slot(const Key& k, uint32_t dflt) const {  // an untouched sibling: its slot, or the default of its kind
        const uint32_t* s = S.find_slot(k);
        return s ? *s : dflt;
    }
    Val hashed(const Key& dst_key, const std::vector<uint32_t>& in, uint32_t level) {
        const uint32_t dst = slot_for(dst_key);
        P.nodes.push_back({dst, (uint32_t)P.inputs.size(), (uint32_t)in.size(), level});
        P.inputs.insert(P.inputs.end(), in.begin(), in.end());
        return {dst, level};
    }
    // the value at `prefix` (of model type m, prefix.size() == d) given the sorted pairs [lo, hi) below it (non-empty)
    Val build(int m, uint64_t d, uint64_t lo, uint64_t hi) {
        const auto& n = S.M.nodes[m];
        if (!P.err.empty()) return {0, 0};
        if (n.kind == 0) {
            if (hi - lo != 1) { P.err = "duplicate locator"; P.code = BZK_REFUSE_DUPLICATE_LOCATOR; return {0, 0}; }
            if (len(lo) != d) { P.err = "locator points below a scalar (ZkLocatorError::InvalidLocator)"; P.code = BZK_REFUSE_INVALID_LOCATOR; return {0, 0}; }
            const uint32_t s = slot_for(prefix);
            P.scalar_dst[order[lo]] = s;
            return {s, 0};
        }
        for (uint64_t i = lo; i < hi; ++i)
            if (len(i) <= d) { P.err = "locator does not reach a scalar (StateManagerError::NonScalarLocatorError)"; P.code = BZK_REFUSE_NON_SCALAR_LOCATOR; return {0, 0}; }
        if (n.kind == 1) {
            std::vector<uint32_t> in(n.fields.size());
            uint32_t lv = 0;
            uint64_t i = lo;
            for (size_t f = 0; f < n.fields.size(); ++f) {
                uint64_t j = i;
                while (j < hi && at(j, d) == f) ++j;
                prefix.push_back(f);
                if (j > i) {
                    const Val v = build(n.fields[f], d + 1, i, j);
                    in[f] = v.slot;
                    lv = std::max(lv, v.level);
                } else {
                    in[f] = read_slot(prefix, S.dflt_slot[n.fields[f]]);
                }
                prefix.pop_back();
                i = j;
            }
            if (i != hi) { P.err = "struct field index out of range (the reference indexes field_types out of bounds)"; P.code = BZK_REFUSE_INVALID_LOCATOR; return {0, 0}; }
            if (!P.err.empty()) return {0, 0};
            return hashed(prefix, in, lv + 1);
        }
        const uint64_t size = n.log4 >= 32 ? ~0ull : ((uint64_t)1 << (2 * n.log4));
        struct Cur { uint64_t idx; Val v; };
        std::vector<Cur> cur;
        for (uint64_t i = lo; i < hi;) {
            const uint64_t idx = at(i, d);
            if (idx >= size) { P.err = "list index out of range (ZkLocatorError::InvalidLocator)"; P.code = BZK_REFUSE_INVALID_LOCATOR; return {0, 0}; }
            uint64_t j = i;
            while (j < hi && at(j, d) == idx) ++j;
            prefix.push_back(idx);
            cur.push_back({idx, build(n.item, d + 1, i, j)});
            prefix.pop_back();
            if (!P.err.empty()) return {0, 0};
            i = j;
        }
        if (n.log4 == 0) {
            // `set_data`'s level loop does not run: the list's value IS its only item; both locators name one slot
            // (this prefix is visited once per plan, so the index alone says whether the alias exists)
            if (!S.find_slot(prefix)) P.new_keys.push_back({prefix, cur[0].v.slot});
            return cur[0].v;
        }
        for (int k = n.log4; k > 0; --k) {  // children at depth k -> parents at depth k - 1
            std::vector<Cur> up;
            for (size_t i = 0; i < cur.size();) {
                const uint64_t parent = cur[i].idx >> 2;
                std::vector<uint32_t> in(4);
                uint32_t lv = 0;
                for (uint64_t j = 0; j < 4; ++j) {
                    const uint64_t child = 4 * parent + j;
                    if (i < cur.size() && cur[i].idx == child) {
                        in[j] = cur[i].v.slot;
                        lv = std::max(lv, cur[i].v.level);
                        ++i;
                    } else {
                        if (k == n.log4) {
                            prefix.push_back(child);
                        } else {
                            prefix.push_back(AUX | (uint64_t)k);
                            prefix.push_back(child);
                        }
                        in[j] = read_slot(prefix, S.depth_slot[m][k]);
                        prefix.resize(d);
                    }
                }
                if (k > 1) {
                    prefix.push_back(AUX | (uint64_t)(k - 1));
                    prefix.push_back(parent);
                }
                const Val v = hashed(prefix, in, lv + 1);
                prefix.resize(d);
                if (!P.err.empty()) return {0, 0};
                up.push_back({parent, v});
            }
            cur.swap(up);
        }
        return cur[0].v;
    }
};

// the pairs of one delta in the order the walk wants them: by locator, a proper prefix first (the walk then reports it)
inline std::vector<uint64_t> sorted_pairs(const uint64_t* loc_off, const uint64_t* loc, uint64_t n) {
    std::vector<uint64_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        return std::lexicographical_compare(loc + loc_off[a], loc + loc_off[a + 1], loc + loc_off[b], loc + loc_off[b + 1]);
    });
    return order;
}

// ---- the chain ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t SRC_ARENA = 0x80000000u;  // source index: the low 31 bits index the round's arena, not the value store
constexpr uint32_t NO_ROOT = 0xffffffffu;    // an empty delta: the state before it
constexpr uint64_t ROUND_VERSIONS_DEFAULT = (uint64_t)1 << 22;
constexpr uint64_t ROUND_VERSIONS_MAX = ((uint64_t)1 << 30) - 1;  // a round of several deltas: every arena index below 2^31 with room to spare
constexpr uint64_t DELTA_VERSIONS_MAX = 0x7ffffff0ull;            // a delta that runs alone

// slot -> a 64-bit value, in pages made on first touch: a call touches few slots of a store that may hold 2^31 (a hash map here cost more than the walk)
struct SlotMap {
    static constexpr uint32_t PAGE = 256;
    std::vector<std::unique_ptr<uint64_t[]>> pages;  // grows with the largest slot that was set
    uint64_t none;
    explicit SlotMap(uint64_t none_) : none(none_) {}
    uint64_t get(uint32_t s) const {
        const size_t q = s / PAGE;
        return q < pages.size() && pages[q] ? pages[q][s % PAGE] : none;
    }
    void set(uint32_t s, uint64_t v) {
        const size_t q = s / PAGE;
        if (q >= pages.size()) pages.resize(std::max(q + 1, 2 * pages.size()));
        if (!pages[q]) {
            pages[q].reset(new uint64_t[PAGE]);
            std::fill(pages[q].get(), pages[q].get() + PAGE, none);
        }
        pages[q][s % PAGE] = v;
    }
};

// the handle's index plus the keys that earlier deltas of this call created
template <class St>
struct Overlay {
    const St& base;
    const decltype(St::M)& M;
    const std::vector<uint32_t>& dflt_slot;
    const std::vector<std::vector<uint32_t>>& depth_slot;
    KeyIndex extra;
    explicit Overlay(const St& s) : base(s), M(s.M), dflt_slot(s.dflt_slot), depth_slot(s.depth_slot) {}
    const uint32_t* find_slot(const Key& k) const {
        auto it = base.slot_of.find(k);
        if (it != base.slot_of.end()) return &it->second;
        auto e = extra.find(k);
        return e != extra.end() ? &e->second : nullptr;
    }
};

struct DeltaPlan {
    UpPlan P;
    uint64_t pair0 = 0, n = 0;  // its pairs: [pair0, pair0 + n) of the call
    uint32_t top_slot = 0;      // n > 0: the slot of the model's root
    uint32_t used_after = 0;    // slots handed out once it is applied
    uint64_t size_after = 0;    // `state_size` once it is applied
    uint64_t versions() const { return n + P.nodes.size(); }
};

// where prev_values_out of a pair comes from
constexpr int64_t PREV_RESIDENT = -1, PREV_ZERO = -2;  // >= 0: the value of that earlier pair of the call

template <class St>
struct ChainPlanner {
    const St& S;
    Overlay<St> ov;
    std::vector<DeltaPlan> deltas;  // the deltas before the first refused one
    bool refused = false;           // delta deltas.size() is refused: why
    int32_t refuse_code = 0;
    std::string refuse_err;
    std::vector<int64_t> prev_of;  // per pair of the planned deltas
    explicit ChainPlanner(const St& s) : S(s), ov(s) {}

    // plans delta after delta until one is refused.  canon(32 bytes) -> is a canonical field element.  loc_off: the CSR of ALL pairs of the call
    template <class Canon>
    void plan(uint64_t m, const uint64_t* delta_off, const uint64_t* loc_off, const uint64_t* loc, const uint8_t* values, Canon canon) {
        uint32_t next_slot = (uint32_t)S.used;
        uint64_t size = S.size;
        const uint64_t NONE = ~(uint64_t)0;
        SlotMap nz(NONE);         // zero / non-zero of the scalar slots this call wrote, over S.nonzero
        SlotMap last_pair(NONE);  // slot -> the latest pair that wrote it
        auto refuse = [&](int32_t code, const std::string& why) {
            refused = true;
            refuse_code = code;
            refuse_err = why;
        };
        for (uint64_t j = 0; j < m && !refused; ++j) {
            DeltaPlan D;
            D.pair0 = delta_off[j];
            D.n = delta_off[j + 1] - delta_off[j];
            if (D.n >= 0x3fffffffull) { refuse(BZK_REFUSE_OTHER, "too many pairs"); break; }
            for (uint64_t i = 0; i < D.n && !refused; ++i)
                if (!canon(values + 32 * (D.pair0 + i))) refuse(BZK_REFUSE_NON_CANONICAL_VALUE, "a value is not a canonical field element");
            if (refused) break;
            D.P.next_slot = next_slot;
            if (D.n) {
                const uint64_t* lo = loc_off + D.pair0;
                const std::vector<uint64_t> order = sorted_pairs(lo, loc, D.n);
                D.P.scalar_dst.assign(D.n, 0);
                Updater<Overlay<St>> U{ov, D.P, lo, loc, order, {}};
                D.top_slot = U.build(S.M.root, 0, 0, D.n).slot;
                if (D.P.err.empty() && D.versions() >= DELTA_VERSIONS_MAX) { D.P.err = "too many nodes"; D.P.code = BZK_REFUSE_OTHER; }
                if (!D.P.err.empty()) { refuse(D.P.code, D.P.err); break; }
                for (auto& nk : D.P.new_keys) ov.extra.emplace(nk.first, nk.second);
                next_slot = D.P.next_slot;
                for (uint64_t i = 0; i < D.n; ++i) {
                    const uint32_t s = D.P.scalar_dst[i];
                    const uint8_t* v = values + 32 * (D.pair0 + i);
                    bool now = false;
                    for (int b = 0; b < 32; ++b) now |= v[b] != 0;
                    const uint64_t seen = nz.get(s);
                    const bool was = seen != NONE ? seen != 0 : (s < S.used && S.nonzero[s]);
                    if (now && !was) ++size;
                    if (!now && was) --size;
                    nz.set(s, now ? 1 : 0);
                    const uint64_t lp = last_pair.get(s);
                    prev_of.push_back(lp != NONE ? (int64_t)lp : s < S.used ? PREV_RESIDENT : PREV_ZERO);
                    last_pair.set(s, D.pair0 + i);
                }
            }
            D.used_after = next_slot;
            D.size_after = size;
            deltas.push_back(std::move(D));
        }
    }

    // whole deltas while the versions stay at most round_versions; a larger delta runs alone
    std::vector<uint64_t> rounds(uint64_t round_versions) const {
        const uint64_t cap = std::min(round_versions ? round_versions : ROUND_VERSIONS_DEFAULT, ROUND_VERSIONS_MAX);
        return cut_rounds((uint64_t)deltas.size(), ~(uint64_t)0, cap, [&](uint64_t j) { return deltas[j].versions(); });
    }
};

// one round, resolved: what goes up, what is launched, where the roots lie, what a commit writes
struct ChainRound {
    uint64_t d0 = 0, d1 = 0;       // its deltas
    uint64_t pair0 = 0, n_up = 0;  // the pairs whose values are the arena's front
    uint64_t n_versions = 0;       // the arena's length
    struct Group { uint32_t arity, level; uint64_t count, src_off, first; };  // outputs at arena[first .. first + count), inputs src[src_off ..)
    std::vector<Group> groups;       // lowest level first
    std::vector<uint32_t> src;       // source indices: per group, per node, its `arity` inputs
    std::vector<uint32_t> root_ix;   // per delta: the arena index of the state hash after it, NO_ROOT for an empty delta
    struct Write { uint32_t delta, slot, arena; };
    std::vector<Write> writes;       // every version in delta order: delta (index in the call), its slot, its arena index
    uint64_t widest_in = 0;          // the largest count * arity of a group with arity > 7 (those run as gather, hash, no fused kernel)

    void resolve(const std::vector<DeltaPlan>& deltas, uint64_t a, uint64_t b) {
        d0 = a, d1 = b;
        pair0 = deltas[a].pair0;
        n_up = deltas[b - 1].pair0 + deltas[b - 1].n - pair0;
        // temporary version ids: kind in the high word (0 resident slot, 1 arena index of an uploaded scalar, 2 node of this round in creation order)
        const uint64_t K_UP = (uint64_t)1 << 32, K_NODE = (uint64_t)2 << 32;
        const uint64_t NONE = ~(uint64_t)0;
        SlotMap latest(NONE);  // slot -> its latest version so far
        struct RNode { uint32_t arity, level, delta, slot; uint64_t first_in; };
        std::vector<RNode> nodes;
        std::vector<uint64_t> tin;
        std::vector<uint64_t> roots(b - a, 0);
        std::vector<std::pair<uint32_t, uint64_t>> wtmp;  // (delta, slot) with the temporary id
        std::vector<uint32_t> wslot;
        for (uint64_t j = a; j < b; ++j) {
            const DeltaPlan& D = deltas[j];
            for (uint64_t i = 0; i < D.n; ++i) {
                const uint64_t v = K_UP | (D.pair0 + i - pair0);
                latest.set(D.P.scalar_dst[i], v);
                wtmp.push_back({(uint32_t)j, v});
                wslot.push_back(D.P.scalar_dst[i]);
            }
            for (const UpPlan::Node& x : D.P.nodes) {  // creation order: children before parents
                uint32_t lv = 0;
                const uint64_t first_in = tin.size();
                for (uint32_t k = 0; k < x.arity; ++k) {
                    const uint32_t s = D.P.inputs[x.first_in + k];
                    const uint64_t seen = latest.get(s);
                    const uint64_t v = seen != NONE ? seen : (uint64_t)s;
                    if ((v >> 32) == 2) lv = std::max(lv, nodes[(uint32_t)v].level);
                    tin.push_back(v);
                }
                const uint64_t v = K_NODE | (uint64_t)nodes.size();
                nodes.push_back({x.arity, lv + 1, (uint32_t)j, x.dst, first_in});
                latest.set(x.dst, v);
                wtmp.push_back({(uint32_t)j, v});
                wslot.push_back(x.dst);
            }
            roots[j - a] = D.n ? latest.get(D.top_slot) : NONE;
        }
        // groups of equal (level, arity), lowest level first: a node's arena index = n_up + its rank in that order
        const size_t nn = nodes.size();
        // (a counting sort, stable in creation order: levels and arities are small numbers, the nodes of a long chain are millions)
        std::vector<uint32_t> by(nn), rank(nn);
        {
            uint32_t top = 0;
            for (const RNode& x : nodes) top = std::max(top, x.level);
            std::vector<uint64_t> start(((size_t)top + 1) * 17 + 1, 0);
            for (const RNode& x : nodes) ++start[(size_t)x.level * 17 + x.arity + 1];
            for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
            for (size_t i = 0; i < nn; ++i) by[start[(size_t)nodes[i].level * 17 + nodes[i].arity]++] = (uint32_t)i;
        }
        for (size_t r = 0; r < nn; ++r) rank[by[r]] = (uint32_t)r;
        n_versions = n_up + nn;
        auto final_ix = [&](uint64_t v) -> uint32_t {  // an arena index
            return (v >> 32) == 2 ? (uint32_t)(n_up + rank[(uint32_t)v]) : (uint32_t)v;
        };
        groups.clear();
        src.clear();
        src.reserve(tin.size());
        widest_in = 0;
        for (size_t r = 0; r < nn;) {
            const RNode& g = nodes[by[r]];
            size_t e = r;
            while (e < nn && nodes[by[e]].level == g.level && nodes[by[e]].arity == g.arity) ++e;
            groups.push_back({g.arity, g.level, (uint64_t)(e - r), (uint64_t)src.size(), n_up + r});
            for (size_t q = r; q < e; ++q) {
                const RNode& x = nodes[by[q]];
                for (uint32_t k = 0; k < x.arity; ++k) {
                    const uint64_t v = tin[x.first_in + k];
                    src.push_back((v >> 32) ? (SRC_ARENA | final_ix(v)) : (uint32_t)v);
                }
            }
            if (g.arity > 7) widest_in = std::max<uint64_t>(widest_in, (uint64_t)(e - r) * g.arity);
            r = e;
        }
        root_ix.assign(b - a, NO_ROOT);
        for (uint64_t j = a; j < b; ++j)
            if (deltas[j].n) root_ix[j - a] = final_ix(roots[j - a]);
        writes.clear();
        writes.reserve(wtmp.size());
        for (size_t i = 0; i < wtmp.size(); ++i) writes.push_back({wtmp[i].first, wslot[i], final_ix(wtmp[i].second)});
    }

    // the commit of deltas [d0, upto): per written slot its latest version before `upto` - no slot twice
    void commit_lists(uint64_t upto, std::vector<uint32_t>& from_arena, std::vector<uint32_t>& to_slot) const {
        from_arena.clear();
        to_slot.clear();
        const uint64_t NONE = ~(uint64_t)0;
        SlotMap at(NONE);  // slot -> position in the lists
        for (const Write& w : writes) {
            if (w.delta >= upto) break;
            const uint64_t seen = at.get(w.slot);
            if (seen != NONE) {
                from_arena[(size_t)seen] = w.arena;
            } else {
                at.set(w.slot, to_slot.size());
                to_slot.push_back(w.slot);
                from_arena.push_back(w.arena);
            }
        }
    }
};

// the host's half of a commit of deltas [d0, upto) (upto > d0): index entries, zero / non-zero bits, size, slots - and nothing of what lies behind
template <class St>
void commit_index(St& S, std::vector<DeltaPlan>& deltas, uint64_t d0, uint64_t upto, const uint8_t* values) {
    S.used = deltas[upto - 1].used_after;
    S.nonzero.resize(S.used, 0);
    for (uint64_t j = d0; j < upto; ++j) {
        DeltaPlan& D = deltas[j];
        for (auto& nk : D.P.new_keys) S.slot_of.emplace(std::move(nk.first), nk.second);
        D.P.new_keys.clear();
        for (uint64_t i = 0; i < D.n; ++i) {
            const uint8_t* v = values + 32 * (D.pair0 + i);
            bool now = false;
            for (int b = 0; b < 32; ++b) now |= v[b] != 0;
            S.nonzero[D.P.scalar_dst[i]] = now ? 1 : 0;
        }
    }
    S.size = deltas[upto - 1].size_after;
}

}  // namespace sc
}  // namespace bzk
