// Stand-alone check of the chain planner (bazuka_amd/csrc/bzk_state_chain.h) without a GPU: the planner runs against a value store in host memory,
// every group is executed with poseidon29_hash<T> on the host (the function the kernels call), and the result is held against the states that
// tests/pystate.py::PyKvState gives after every delta (read from the case file that tests/test_state_chain_cpu.py writes).  Built with the address
// and undefined-behaviour sanitizers (host code only).
//   usage: _state_chain_check <case file>
// Case file, little endian: u64 cases; per case: u64 model length + bincode(ZkStateModel); u64 m; per delta u64 pairs, per pair u64 locator length,
// the locator's u64s, 32 bytes of value; u64 refused_at (m: none); per delta before refused_at: 32 bytes state hash, u64 state size.
// Every case runs with round_versions 0 (the default), 1, exactly the version count of its first non-empty delta, and one less; with the true claims;
// with no claims; and with a wrong claim at its first, a middle and its last delta.  After every run: every intermediate state, verdicts, and the
// committed state (store, index, non-zero bits, size, slots) equal to the one the same planner leaves after the applied deltas ONE CALL EACH (m = 1).
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../bazuka_amd/csrc/bzk_field.cuh"
#include "../../bazuka_amd/csrc/bzk_poseidon29.cuh"
#include "../../bazuka_amd/csrc/bzk_state_chain.h"

namespace bzk {
int32_t poseidon_consts_host29(int t, const Fr29** out, int* rf, int* rp);  // poseidon.hip (libbzk.so): host memory, no device
}
using namespace bzk;

#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); \
            fprintf(stderr, __VA_ARGS__);               \
            fprintf(stderr, "\n");                      \
            exit(1);                                    \
        }                                               \
    } while (0)

static Fr hash_host(const Fr* in, int arity) {
    const Fr29* c;
    int rf, rp;
    CHECK(poseidon_consts_host29(arity + 1, &c, &rf, &rp) == 0, "no constants for width %d", arity + 1);
    switch (arity + 1) {
        case 2: return poseidon29_hash<2>(in, c, rf, rp);
        case 3: return poseidon29_hash<3>(in, c, rf, rp);
        case 4: return poseidon29_hash<4>(in, c, rf, rp);
        case 5: return poseidon29_hash<5>(in, c, rf, rp);
        case 6: return poseidon29_hash<6>(in, c, rf, rp);
        case 7: return poseidon29_hash<7>(in, c, rf, rp);
        default: return poseidon29_hash<8>(in, c, rf, rp);
    }
}

struct MNode {
    int kind = 0;
    std::vector<int> fields;
    int log4 = 0, item = -1;
    Fr dflt;
    std::vector<Fr> list_dflt;
};
struct HModel {
    std::vector<MNode> nodes;
    int root = -1;
};
struct Rd {
    const uint8_t* p;
    size_t len, off = 0;
    uint64_t u(int bytes) {
        CHECK(off + bytes <= len, "case file truncated at %zu", off);
        uint64_t v = 0;
        for (int i = 0; i < bytes; ++i) v |= (uint64_t)p[off + i] << (8 * i);
        off += bytes;
        return v;
    }
    const uint8_t* take(size_t n) {
        CHECK(off + n <= len, "case file truncated at %zu", off);
        off += n;
        return p + off - n;
    }
};
static int parse_model(Rd& r, HModel& M) {
    const uint64_t tag = r.u(4);
    const int id = (int)M.nodes.size();
    M.nodes.emplace_back();
    if (tag == 1) {
        const uint64_t k = r.u(8);
        CHECK(k >= 1 && k <= 7, "the check hashes widths 2 .. 8");
        std::vector<int> f;
        for (uint64_t i = 0; i < k; ++i) f.push_back(parse_model(r, M));
        M.nodes[id].kind = 1;
        M.nodes[id].fields = f;
    } else if (tag == 2) {
        const int lg = (int)r.u(1);
        const int c = parse_model(r, M);
        M.nodes[id].kind = 2;
        M.nodes[id].log4 = lg;
        M.nodes[id].item = c;
    } else {
        CHECK(tag == 0, "model tag");
    }
    return id;
}
static void model_defaults(HModel& M, int id) {
    if (M.nodes[id].kind == 0) {
        M.nodes[id].dflt = Fr::zero();
    } else if (M.nodes[id].kind == 1) {
        std::vector<Fr> v;
        for (int f : std::vector<int>(M.nodes[id].fields)) {
            model_defaults(M, f);
            v.push_back(M.nodes[f].dflt);
        }
        M.nodes[id].dflt = hash_host(v.data(), (int)v.size());
    } else {
        model_defaults(M, M.nodes[id].item);
        MNode& n = M.nodes[id];
        n.list_dflt.assign((size_t)n.log4 + 1, Fr::zero());
        n.list_dflt[n.log4] = M.nodes[n.item].dflt;
        for (int k = n.log4 - 1; k >= 0; --k) {
            const Fr c[4] = {n.list_dflt[k + 1], n.list_dflt[k + 1], n.list_dflt[k + 1], n.list_dflt[k + 1]};
            n.list_dflt[k] = hash_host(c, 4);
        }
        n.dflt = n.list_dflt[0];
    }
}

// the members bzk_state_chain.h reads, and the value store in host memory
struct HState {
    HModel M;
    std::vector<uint32_t> dflt_slot;
    std::vector<std::vector<uint32_t>> depth_slot;
    sc::KeyIndex slot_of;
    size_t used = 0;
    std::vector<uint8_t> nonzero;
    uint64_t size = 0, height = 0;
    std::vector<Fr> vals;
    Fr root;
    const uint32_t* find_slot(const sc::Key& k) const {
        auto it = slot_of.find(k);
        return it != slot_of.end() ? &it->second : nullptr;
    }
    explicit HState(const HModel& m) : M(m) {  // as bzk_state_create lays the defaults out
        dflt_slot.assign(M.nodes.size(), 0);
        depth_slot.assign(M.nodes.size(), {});
        for (size_t i = 0; i < M.nodes.size(); ++i) {
            dflt_slot[i] = (uint32_t)vals.size();
            vals.push_back(M.nodes[i].dflt);
            if (M.nodes[i].kind == 2)
                for (int k = 0; k <= M.nodes[i].log4; ++k) {
                    depth_slot[i].push_back((uint32_t)vals.size());
                    vals.push_back(M.nodes[i].list_dflt[k]);
                }
        }
        used = vals.size();
        nonzero.assign(used, 0);
        root = M.nodes[M.root].dflt;
    }
};

struct Case {
    HModel M;
    uint64_t m = 0, refused_at = 0;
    std::vector<uint64_t> delta_off, loc_off, loc, heights;
    std::vector<uint8_t> values, want;  // want: 40 bytes per delta before refused_at
};

static bool canonical(const uint8_t* v) {
    Fr f;
    memcpy(f.l, v, 32);
    Fr g = f;
    fe_reduce_once<FrParams>(g);
    return g.equals(f);
}

struct Outcome {
    std::vector<uint8_t> states, verdict;
    uint64_t applied = 0;
};

// state.hip's state_chain_impl with the launches as loops
static Outcome run_chain(HState& S, const Case& C, uint64_t first, uint64_t m, const uint8_t* claims, uint64_t round_versions, uint64_t* first_versions) {
    Outcome O;
    O.states.assign(m * 40, 0);
    O.verdict.assign(m, BZK_CHAIN_NOT_REACHED);
    std::vector<uint64_t> d_off(C.delta_off.begin() + first, C.delta_off.begin() + first + m + 1);
    sc::ChainPlanner<HState> PL(S);
    PL.plan(m, d_off.data(), C.loc_off.data(), C.loc.data(), C.values.data(), canonical);
    const uint64_t mp = PL.deltas.size();
    if (first_versions)
        for (auto& D : PL.deltas)
            if (D.n) { *first_versions = D.versions(); break; }
    const std::vector<uint64_t> cuts = PL.rounds(round_versions);
    bool stopped = false;
    for (size_t r = 0; r + 1 < cuts.size() && !stopped; ++r) {
        sc::ChainRound R;
        R.resolve(PL.deltas, cuts[r], cuts[r + 1]);
        uint64_t weight = 0;
        for (uint64_t j = R.d0; j < R.d1; ++j) weight += PL.deltas[j].versions();
        CHECK(weight == R.n_versions, "a round's arena holds its deltas' versions");
        const uint64_t cap = round_versions ? round_versions : sc::ROUND_VERSIONS_DEFAULT;
        CHECK(R.d1 - R.d0 == 1 || weight <= cap, "round of %llu versions over the limit %llu", (unsigned long long)weight, (unsigned long long)cap);
        std::vector<Fr> arena(R.n_versions);
        std::vector<uint8_t> written(R.n_versions, 0);
        for (uint64_t i = 0; i < R.n_up; ++i) {
            memcpy(arena[i].l, C.values.data() + 32 * (R.pair0 + i), 32);
            written[i] = 1;
        }
        uint32_t level = 0;
        for (const auto& g : R.groups) {
            CHECK(g.level >= level && g.level >= 1, "groups run lowest level first");
            level = g.level;
            for (uint64_t i = 0; i < g.count; ++i) {
                Fr in[16];
                CHECK(g.arity >= 1 && g.arity <= 7, "width");
                for (uint32_t k = 0; k < g.arity; ++k) {
                    const uint32_t s = R.src[g.src_off + i * g.arity + k];
                    if (s & sc::SRC_ARENA) {
                        const uint32_t a = s & ~sc::SRC_ARENA;
                        CHECK(a < R.n_versions && written[a], "arena source %u not written before level %u", a, g.level);
                        CHECK(a < g.first || a >= g.first + g.count, "a group reads what it writes");
                        in[k] = arena[a];
                    } else {
                        CHECK(s < S.used, "plain source %u beyond the %zu committed slots", s, S.used);
                        in[k] = S.vals[s];
                    }
                }
                CHECK(g.first + i < R.n_versions && !written[g.first + i], "arena position written twice");
                arena[g.first + i] = hash_host(in, (int)g.arity);
            }
            for (uint64_t i = 0; i < g.count; ++i) written[g.first + i] = 1;  // a level becomes visible as a whole, like a launch
        }
        std::vector<uint8_t> states((R.d1 - R.d0) * 40);
        Fr cur = S.root;
        uint64_t upto = R.d1;
        for (uint64_t j = R.d0; j < R.d1; ++j) {
            if (R.root_ix[j - R.d0] != sc::NO_ROOT) {
                CHECK(R.root_ix[j - R.d0] < R.n_versions, "root index");
                cur = arena[R.root_ix[j - R.d0]];
            }
            uint8_t* s40 = states.data() + 40 * (j - R.d0);
            memcpy(s40, cur.l, 32);
            memcpy(s40 + 32, &PL.deltas[j].size_after, 8);
            if (upto == R.d1 && claims && memcmp(s40, claims + 40 * j, 40) != 0) upto = j;
        }
        if (upto > R.d0) {
            std::vector<uint32_t> from, dst;
            R.commit_lists(upto, from, dst);
            S.vals.resize(PL.deltas[upto - 1].used_after, Fr::zero());
            std::vector<uint8_t> hit(S.vals.size(), 0);
            for (size_t i = 0; i < dst.size(); ++i) {
                CHECK(dst[i] < S.vals.size() && from[i] < R.n_versions && !hit[dst[i]], "commit lists: in range, no slot twice");
                hit[dst[i]] = 1;
                S.vals[dst[i]] = arena[from[i]];
            }
            sc::commit_index(S, PL.deltas, R.d0, upto, C.values.data());
            memcpy(S.root.l, states.data() + 40 * (upto - 1 - R.d0), 32);
            S.height = C.heights[first + upto - 1];
            O.applied = upto;
        }
        const uint64_t shown = upto < R.d1 ? upto + 1 : upto;
        memcpy(O.states.data() + 40 * R.d0, states.data(), (shown - R.d0) * 40);
        for (uint64_t j = R.d0; j < upto; ++j) O.verdict[j] = BZK_CHAIN_APPLIED;
        if (upto < R.d1) {
            O.verdict[upto] = BZK_CHAIN_MISMATCH;
            stopped = true;
        }
    }
    if (!stopped && PL.refused) O.verdict[mp] = BZK_CHAIN_REFUSED;
    return O;
}

static void same_state(const HState& A, const HState& B, const char* what) {
    CHECK(A.used == B.used && A.vals.size() == B.vals.size(), "%s: %zu slots against %zu", what, A.used, B.used);
    for (size_t i = 0; i < A.vals.size(); ++i) CHECK(A.vals[i].equals(B.vals[i]), "%s: slot %zu differs", what, i);
    CHECK(A.slot_of == B.slot_of, "%s: index differs (%zu keys against %zu)", what, A.slot_of.size(), B.slot_of.size());
    CHECK(A.nonzero == B.nonzero && A.size == B.size && A.height == B.height && A.root.equals(B.root), "%s: size / height / root / bits", what);
}

int main(int argc, char** argv) {
    CHECK(argc == 2, "usage: %s <case file>", argv[0]);
    FILE* f = fopen(argv[1], "rb");
    CHECK(f, "cannot open %s", argv[1]);
    std::vector<uint8_t> bytes;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + k);
    fclose(f);
    Rd r{bytes.data(), bytes.size()};
    const uint64_t n_cases = r.u(8);
    uint64_t runs = 0, rounds_seen = 0;
    for (uint64_t c = 0; c < n_cases; ++c) {
        Case C;
        const uint64_t ml = r.u(8);
        Rd mr{r.take(ml), (size_t)ml};
        C.M.root = parse_model(mr, C.M);
        CHECK(mr.off == ml, "model bytes");
        model_defaults(C.M, C.M.root);
        C.m = r.u(8);
        C.delta_off.push_back(0);
        C.loc_off.push_back(0);
        for (uint64_t j = 0; j < C.m; ++j) {
            const uint64_t n = r.u(8);
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t k = r.u(8);
                for (uint64_t q = 0; q < k; ++q) C.loc.push_back(r.u(8));
                C.loc_off.push_back(C.loc.size());
                const uint8_t* v = r.take(32);
                C.values.insert(C.values.end(), v, v + 32);
            }
            C.delta_off.push_back(C.delta_off.back() + n);
            C.heights.push_back(100 + 3 * j);
        }
        if (C.loc.empty()) C.loc.push_back(0);
        if (C.values.empty()) C.values.resize(32);
        C.refused_at = r.u(8);
        CHECK(C.refused_at <= C.m, "refused_at");
        const uint8_t* w = r.take(40 * C.refused_at);
        C.want.assign(w, w + 40 * C.refused_at);
        C.want.resize(40 * C.m, 0xEE);  // claims behind a refused delta are never looked at

        // the yardstick of the committed state: the same planner, one delta per call
        std::vector<HState> seq;  // seq[k]: after k deltas
        seq.emplace_back(C.M);
        for (uint64_t j = 0; j < C.refused_at; ++j) {
            HState S = seq.back();
            const Outcome O = run_chain(S, C, j, 1, nullptr, 0, nullptr);
            CHECK(O.applied == 1 && O.verdict[0] == BZK_CHAIN_APPLIED, "case %llu: delta %llu alone", (unsigned long long)c, (unsigned long long)j);
            CHECK(memcmp(O.states.data(), C.want.data() + 40 * j, 40) == 0, "case %llu: delta %llu alone gives another state than the restatement",
                  (unsigned long long)c, (unsigned long long)j);
            seq.push_back(std::move(S));
        }
        if (C.refused_at < C.m) {
            HState S = seq.back();
            const Outcome O = run_chain(S, C, C.refused_at, 1, nullptr, 0, nullptr);
            CHECK(O.applied == 0 && O.verdict[0] == BZK_CHAIN_REFUSED, "case %llu: the refused delta alone", (unsigned long long)c);
            same_state(S, seq.back(), "a refused delta leaves no trace");
        }
        uint64_t fv = 0;
        {
            HState S(C.M);
            run_chain(S, C, 0, C.m, nullptr, 0, &fv);
        }
        std::vector<uint64_t> rvs = {0, 1};
        if (fv) rvs.push_back(fv);
        if (fv > 1) rvs.push_back(fv - 1);
        std::vector<int64_t> wrong = {-2, -1};  // -2: no claims, -1: the true claims, k: claim k wrong
        if (C.refused_at) {
            wrong.push_back(0);
            wrong.push_back((int64_t)(C.refused_at / 2));
            wrong.push_back((int64_t)C.refused_at - 1);
        }
        for (uint64_t rv : rvs)
            for (int64_t bad : wrong)
                for (int in_size = 0; in_size < (bad >= 0 ? 2 : 1); ++in_size) {
                    std::vector<uint8_t> claims = C.want;
                    if (bad >= 0) claims[40 * bad + (in_size ? 33 : 7)] ^= 0x10;
                    HState S(C.M);
                    const Outcome O = run_chain(S, C, 0, C.m, bad == -2 ? nullptr : claims.data(), rv, nullptr);
                    const uint64_t want_applied = bad >= 0 ? (uint64_t)bad : C.refused_at;
                    CHECK(O.applied == want_applied, "case %llu rv %llu bad %lld: applied %llu, expected %llu", (unsigned long long)c, (unsigned long long)rv,
                          (long long)bad, (unsigned long long)O.applied, (unsigned long long)want_applied);
                    for (uint64_t j = 0; j < C.m; ++j) {
                        const uint8_t v = j < want_applied ? BZK_CHAIN_APPLIED
                                          : j > want_applied ? BZK_CHAIN_NOT_REACHED
                                          : bad >= 0 ? BZK_CHAIN_MISMATCH : BZK_CHAIN_REFUSED;
                        CHECK(O.verdict[j] == v, "case %llu rv %llu bad %lld: verdict[%llu] = %u, expected %u", (unsigned long long)c, (unsigned long long)rv,
                              (long long)bad, (unsigned long long)j, O.verdict[j], v);
                        const bool shown = j < want_applied || (j == want_applied && bad >= 0);
                        if (shown) CHECK(memcmp(O.states.data() + 40 * j, C.want.data() + 40 * j, 40) == 0, "case %llu rv %llu bad %lld: state after delta %llu",
                                         (unsigned long long)c, (unsigned long long)rv, (long long)bad, (unsigned long long)j);
                        else for (int b = 0; b < 40; ++b) CHECK(O.states[40 * j + b] == 0, "states_out is zero where nothing is shown");
                    }
                    same_state(S, seq[want_applied], "chain against one call per delta");
                    ++runs;
                }
        rounds_seen += rvs.size();
    }
    CHECK(r.off == bytes.size(), "bytes after the last case");
    printf("state_chain_check ok: %llu cases, %llu runs\n", (unsigned long long)n_cases, (unsigned long long)runs);
    (void)rounds_seen;
    return 0;
}
