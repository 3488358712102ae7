// Wire-form ContractUpdate check (bzk_contract_updates_check): what `update_contract` (src/blockchain/ops/apply_tx/update_contract/mod.rs:28-116)
// computes and verifies per ContractUpdate of one contract - commitment, aux data, every deposit's signature, the proof - for the updates of m
// consecutive transactions.  The parser is host_bincode.h's parse_contract_updates (structure only); the per-lane functions are
// bzk_updates.cuh's; this file holds the plan (rounds, trees, key groups: host arithmetic on counts), the kernels and the two runners.  The
// device runner and the host-thread runner execute the same per-lane functions over the same plan.
//
// Stage 1, per round of at most upd::ROUND_PAYMENTS payments / upd::ROUND_BYTES record bytes (an update is never split):
//   upd_deposit_sig    one lane per payment   Ed25519 verdict of a deposit (the verifier's own register and LDS profile: nothing else is fused in)
//   upd_deposit_leaf   one lane per payment   H4(1, token, amount, calldata)
//   upd_withdraw_leaf  one lane per payment   fingerprint (SHA3-256 with the calldata blanked), H7(1, token, amount, fee token, fee, fingerprint, calldata)
//   upd_tree_level     one launch per level over ALL updates of the round; only parents with a populated child are computed
//   upd_inputs         one lane per update    commitment, aux (root / default / H2 of a FunctionCall), SIGS and ROUTE bits, the five inputs and the
//                                             proof into the update's key group
// Stage 2, all key groups side by side: verify_keys.hip's three kernels over the groups' inputs and proofs, one set of launches per round of 2^16 lanes.
// Stage 3: upd_verdict scatters the group verdicts back to update order and ORs in the bits.
// Aux values, commitments, bits and the groups' arrays of all n updates stay on the device between rounds; everything is one WsLayout.
#include <memory>

#include "bzk_updates.cuh"
#include "bzk_internal.h"
#include "host_bincode.h"
#include "host_pairing.h"
#include "host_threads.h"

namespace bzk {

int32_t poseidon_consts_dev_shared(bzk_ctx* ctx, int t, const void** out, int* rf, int* rp);  // poseidon.hip
int32_t poseidon_consts_host29(int t, const Fr29** out, int* rf, int* rp);          // poseidon.hip

namespace {

using upd::PayRec;
using upd::UpdRec;

constexpr int UPD_SIG_BLOCK = 64;    // one wave per block, a lane's table in its LDS column: ed25519_verify_kernel's shape
constexpr int UPD_HASH_BLOCK = 128;  // poseidon29_kernel's shape

// data: the round's record bytes, whose first byte is byte `base` of the call's updates; rec / pay: the round's updates and payments, pay[i].upd
// counted from the call's first update and upd0 the round's first
__global__ void __launch_bounds__(UPD_SIG_BLOCK) upd_deposit_sig_kernel(const uint8_t* __restrict__ data, uint64_t base, const UpdRec* __restrict__ rec,
                                                                        uint32_t upd0, const PayRec* __restrict__ pay, uint32_t np,
                                                                        const uint32_t* __restrict__ base_tab, uint8_t* __restrict__ sig) {
    __shared__ uint32_t lds[ed25519::LANE_WORDS * UPD_SIG_BLOCK];
    const uint32_t i = blockIdx.x * UPD_SIG_BLOCK + threadIdx.x;
    if (i >= np) return;
    const PayRec p = pay[i];
    const UpdRec& u = rec[p.upd - upd0];
    if (u.kind != upd::DEPOSIT) return;
    sig[i] = upd::deposit_sig(data + (u.at - base) + p.off, p, base_tab, lds + threadIdx.x, UPD_SIG_BLOCK);
}
// leaves: node i of level 0 is payment i of the round; payments of updates without ROUTE have no tree and are left alone
__global__ void __launch_bounds__(UPD_HASH_BLOCK) upd_deposit_leaf_kernel(const uint8_t* __restrict__ data, uint64_t base, const UpdRec* __restrict__ rec,
                                                                          uint32_t upd0, const PayRec* __restrict__ pay, uint32_t np, upd::Consts c,
                                                                          Fr* __restrict__ nodes) {
    const uint32_t i = blockIdx.x * UPD_HASH_BLOCK + threadIdx.x;
    if (i >= np) return;
    const PayRec p = pay[i];
    const UpdRec& u = rec[p.upd - upd0];
    if (u.kind != upd::DEPOSIT || !u.route) return;
    nodes[i] = upd::deposit_leaf(data + (u.at - base) + p.off, p, c);
}
__global__ void __launch_bounds__(UPD_HASH_BLOCK) upd_withdraw_leaf_kernel(const uint8_t* __restrict__ data, uint64_t base, const UpdRec* __restrict__ rec,
                                                                           uint32_t upd0, const PayRec* __restrict__ pay, uint32_t np, upd::Consts c,
                                                                           Fr* __restrict__ nodes) {
    const uint32_t i = blockIdx.x * UPD_HASH_BLOCK + threadIdx.x;
    if (i >= np) return;
    const PayRec p = pay[i];
    const UpdRec& u = rec[p.upd - upd0];
    if (u.kind != upd::WITHDRAW || !u.route) return;
    nodes[i] = upd::withdraw_leaf(data + (u.at - base) + p.off, p, c);
}
// level k >= 1 of every tree of the round: below / row are rows k - 1 and k of the plan, below_at / row_at where those levels' nodes start
__global__ void __launch_bounds__(UPD_HASH_BLOCK) upd_tree_level_kernel(Fr* __restrict__ nodes, const UpdRec* __restrict__ rec,
                                                                        const uint32_t* __restrict__ below, const uint32_t* __restrict__ row, uint32_t mu,
                                                                        uint32_t below_at, uint32_t row_at, uint32_t k, uint32_t lanes, upd::Consts c) {
    const uint32_t i = blockIdx.x * UPD_HASH_BLOCK + threadIdx.x;
    if (i >= lanes) return;
    upd::tree_parent_one(nodes, rec, below, row, mu, below_at, row_at, k, i, c);
}
// one lane per update of the round.  prev_first: the state the round's first update is checked against; a later one reads its predecessor's
// record.  aux / commit / bits: the call's arrays, indexed from the call's first update
__global__ void __launch_bounds__(UPD_HASH_BLOCK) upd_inputs_kernel(const uint8_t* __restrict__ data, uint64_t base, const UpdRec* __restrict__ rec,
                                                                    uint32_t upd0, uint32_t mu, const uint8_t* __restrict__ prev_first,
                                                                    const Fr* __restrict__ nodes, const uint8_t* __restrict__ sig, uint32_t pay_base,
                                                                    upd::Consts c, Fr* __restrict__ aux, Fr* __restrict__ commit,
                                                                    uint8_t* __restrict__ bits, Fr* __restrict__ inputs, uint8_t* __restrict__ proofs) {
    const uint32_t i = blockIdx.x * UPD_HASH_BLOCK + threadIdx.x;
    if (i >= mu) return;
    const UpdRec u = rec[i];
    const uint8_t* prev = i ? data + (rec[i - 1].at - base) + rec[i - 1].next_off : prev_first;
    Fr a, cm;
    upd::inputs_one(data + (u.at - base), u, prev, nodes, c, a, cm, inputs, proofs);
    aux[upd0 + i] = a;
    commit[upd0 + i] = cm;
    bits[upd0 + i] = u.kind == upd::MINT ? (uint8_t)BZK_UPD_UNSUPPORTED
                                         : (uint8_t)((upd::sigs_all(u, sig + (u.pay0 - pay_base)) ? BZK_UPD_SIGS : 0) | (u.route ? BZK_UPD_ROUTE : 0));
}
__global__ void __launch_bounds__(256) upd_verdict_kernel(const uint32_t* __restrict__ slot, const uint8_t* __restrict__ verdict,
                                                          const uint8_t* __restrict__ bits, uint64_t n, uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = slot[i];
    ok[i] = (uint8_t)(bits[i] | ((s != upd::NO_SLOT && verdict[s]) ? BZK_UPD_PROOF : 0));
}

// ---- the plan: everything below is arithmetic on counts and on the function table; no byte of a payment's values is read
struct Group {
    const bzk_contract_fn* fn = nullptr;
    uint64_t first = 0, count = 0;  // its range of the groups' arrays
    hp::KeyHost key;
    std::unique_ptr<hp::KeyUpload> up;
};
struct Round {
    uint64_t u0, u1;      // updates [u0, u1)
    uint32_t depth = 0;   // the deepest tree's capacity
    std::vector<uint32_t> rows;      // (depth + 1) rows of mu + 1 prefix sums: nodes per update and level
    std::vector<uint32_t> level_at;  // depth + 1: where a level's nodes start in the round's node array
    uint32_t n_nodes = 0;
    uint32_t mu() const { return (uint32_t)(u1 - u0); }
    const uint32_t* row(uint32_t k) const { return rows.data() + (size_t)k * (mu() + 1); }
};
struct Plan {
    std::vector<Group> groups;   // deposit functions, withdraw functions, functions: in table order
    std::vector<Round> rounds;
    std::vector<uint32_t> slot;  // n
    uint64_t n_slots = 0;
    std::vector<Fr> dflt;        // upd::Consts::dflt
};
const bzk_contract_fn* function_of(const bzk_contract_desc& c, const UpdRec& u, size_t& group) {
    const bzk_contract_fn* tab[3] = {c.deposit_fns, c.withdraw_fns, c.fns};
    const uint32_t cnt[3] = {c.n_deposit_fns, c.n_withdraw_fns, c.n_fns};
    if (u.kind > upd::CALL || u.circuit_id >= cnt[u.kind]) return nullptr;
    group = (u.kind > 0 ? c.n_deposit_fns : 0) + (u.kind > 1 ? c.n_withdraw_fns : 0) + (size_t)u.circuit_id;
    return tab[u.kind] + u.circuit_id;
}
// ROUTE, heights, key groups, rounds and the rounds' tree rows
void make_plan(const bzk_contract_desc& c, UpdParsed& P, const uint64_t* count, uint64_t m, uint64_t height0, Plan& plan) {
    const uint64_t n = P.rec.size();
    plan.groups.resize((size_t)c.n_deposit_fns + c.n_withdraw_fns + c.n_fns);
    for (uint32_t k = 0; k < c.n_deposit_fns; ++k) plan.groups[k].fn = c.deposit_fns + k;
    for (uint32_t k = 0; k < c.n_withdraw_fns; ++k) plan.groups[(size_t)c.n_deposit_fns + k].fn = c.withdraw_fns + k;
    for (uint32_t k = 0; k < c.n_fns; ++k) plan.groups[(size_t)c.n_deposit_fns + c.n_withdraw_fns + k].fn = c.fns + k;
    std::vector<uint32_t> group_of(n, upd::NO_SLOT);
    uint64_t i = 0;
    for (uint64_t j = 0; j < m; ++j)
        for (uint64_t k = 0; k < count[j]; ++k, ++i) {
            UpdRec& u = P.rec[i];
            u.height = height0 + j;
            size_t g = 0;
            const bzk_contract_fn* fn = function_of(c, u, g);
            if (!fn) continue;
            u.capacity = u.kind == upd::CALL ? 0 : fn->log4_payment_capacity;
            bool route = u.pay_n <= ((uint64_t)1 << (2 * u.capacity));  // batch_set's locator rule: index < 4^capacity
            for (uint32_t q = 0; q < u.pay_n && route; ++q)
                route = (P.pay[u.pay0 + q].flags & (upd::PAY_CONTRACT | upd::PAY_CIRCUIT)) == (upd::PAY_CONTRACT | upd::PAY_CIRCUIT);
            u.route = route ? 1 : 0;
            if (route) {
                group_of[i] = (uint32_t)g;
                ++plan.groups[g].count;
            }
        }
    uint64_t at = 0;
    for (Group& g : plan.groups) {
        g.first = at;
        at += g.count;
        g.count = 0;  // refilled as the slots are dealt
    }
    plan.n_slots = at;
    plan.slot.assign(n, upd::NO_SLOT);
    for (i = 0; i < n; ++i)
        if (group_of[i] != upd::NO_SLOT) {
            Group& g = plan.groups[group_of[i]];
            P.rec[i].slot = plan.slot[i] = (uint32_t)(g.first + g.count++);
        }
    for (uint64_t a = 0; a < n;) {
        uint64_t b = a + 1, pays = P.rec[a].pay_n;
        while (b < n && pays + P.rec[b].pay_n <= upd::ROUND_PAYMENTS && P.end(b) - P.rec[a].at <= upd::ROUND_BYTES) pays += P.rec[b++].pay_n;
        Round R;
        R.u0 = a;
        R.u1 = b;
        const uint32_t mu = R.mu();
        auto has_tree = [&](const UpdRec& u) { return u.route && u.kind != upd::CALL; };
        for (uint64_t q = a; q < b; ++q)
            if (has_tree(P.rec[q])) R.depth = std::max(R.depth, P.rec[q].capacity);
        R.rows.assign((size_t)(R.depth + 1) * (mu + 1), 0);
        R.level_at.assign(R.depth + 1, 0);
        for (uint32_t t = 0; t < mu; ++t) {
            const UpdRec& u = P.rec[a + t];
            uint32_t have = u.pay_n;
            R.rows[t + 1] = R.rows[t] + have;
            for (uint32_t k = 1; k <= R.depth; ++k) {
                uint32_t* r = R.rows.data() + (size_t)k * (mu + 1);
                have = (has_tree(u) && k <= u.capacity) ? (have + 3) / 4 : 0;
                r[t + 1] = r[t] + have;
            }
        }
        for (uint32_t k = 0; k <= R.depth; ++k) {
            R.level_at[k] = R.n_nodes;
            R.n_nodes += R.row(k)[mu];
        }
        for (uint32_t t = 0; t < mu; ++t) {
            UpdRec& u = P.rec[a + t];
            u.root = (has_tree(u) && u.pay_n) ? R.level_at[u.capacity] + R.row(u.capacity)[t] : upd::NO_SLOT;
        }
        plan.rounds.push_back(std::move(R));
        a = b;
    }
    // d_0 = H(0^w), d_{k+1} = H4(d_k, d_k, d_k, d_k)
    plan.dflt.assign(2 * (upd::MAX_CAPACITY + 1), Fr::zero());
    for (int w = 0; w < 2; ++w) {
        ZkScalar z[7], d = poseidon_hash(z, w ? 7 : 4);
        for (uint32_t k = 0; k <= upd::MAX_CAPACITY; ++k) {
            plan.dflt[(size_t)w * (upd::MAX_CAPACITY + 1) + k] = d.v;
            const ZkScalar four[4] = {d, d, d, d};
            d = poseidon_hash(four, 4);
        }
    }
}
void prepare_keys(Plan& plan, bool device) {   // the groups' keys side by side on the host threads
    host_for_each(plan.groups.size(), host_default_threads(), [&](uint64_t i) {
        Group& g = plan.groups[i];
        if (!g.count) return;
        hp::key_prepare(g.fn->vk, g.fn->vk_len, 5, g.key);   // check_proof's five inputs; a key of another shape verifies nothing
        if (g.key.valid && device) g.up.reset(new hp::KeyUpload(g.key));
    });
}

// ---- the same plan on host threads
int32_t run_host(int threads, const UpdParsed& P, const Plan& plan, const uint8_t state0[32], uint8_t* ok, uint8_t* aux_out, uint8_t* commit_out) {
    const uint64_t n = P.rec.size();
    upd::Consts c;
    BZK_TRY(poseidon_consts_host29(3, &c.c3, &c.rf3, &c.rp3));
    BZK_TRY(poseidon_consts_host29(5, &c.c5, &c.rf5, &c.rp5));
    BZK_TRY(poseidon_consts_host29(8, &c.c8, &c.rf8, &c.rp8));
    c.dflt = plan.dflt.data();
    const uint32_t* tab = ed25519::base_table_host();
    std::vector<Fr> aux(n), commit(n), inputs((size_t)5 * plan.n_slots + 1);
    std::vector<uint8_t> bits(n), proofs((size_t)upd::PROOF_BYTES * plan.n_slots + 1), verdict(plan.n_slots + 1), sig;
    std::vector<Fr> nodes;
    for (const Round& R : plan.rounds) {
        const UpdRec* rec = P.rec.data() + R.u0;
        const uint32_t mu = R.mu(), pay_base = rec[0].pay0, np = R.row(0)[mu];
        const PayRec* pay = P.pay.data() + pay_base;
        nodes.resize((size_t)R.n_nodes + 1);
        sig.assign((size_t)np + 1, 0);
        host_for_each(np, threads, [&](uint64_t i) {
            const PayRec& p = pay[i];
            const UpdRec& u = P.rec[p.upd];
            const uint8_t* at = P.bytes + u.at + p.off;
            if (u.kind == upd::DEPOSIT) {
                uint32_t lane[ed25519::LANE_WORDS];
                sig[i] = upd::deposit_sig(at, p, tab, lane, 1);
            }
            if (!u.route) return;
            nodes[i] = u.kind == upd::DEPOSIT ? upd::deposit_leaf(at, p, c) : upd::withdraw_leaf(at, p, c);
        });
        for (uint32_t k = 1; k <= R.depth; ++k)
            host_for_each(R.row(k)[mu], threads, [&](uint64_t i) {
                upd::tree_parent_one(nodes.data(), rec, R.row(k - 1), R.row(k), mu, R.level_at[k - 1], R.level_at[k], k, (uint32_t)i, c);
            });
        host_for_each(mu, threads, [&](uint64_t i) {
            const UpdRec& u = rec[i];
            const uint64_t g = R.u0 + i;
            const uint8_t* prev = g ? P.bytes + P.rec[g - 1].at + P.rec[g - 1].next_off : state0;
            upd::inputs_one(P.bytes + u.at, u, prev, nodes.data(), c, aux[g], commit[g], inputs.data(), proofs.data());
            bits[g] = u.kind == upd::MINT ? (uint8_t)BZK_UPD_UNSUPPORTED
                                          : (uint8_t)((upd::sigs_all(u, sig.data() + (u.pay0 - pay_base)) ? BZK_UPD_SIGS : 0) | (u.route ? BZK_UPD_ROUTE : 0));
        });
    }
    std::vector<G16kGroup> vg;   // every group's rows in one task loop
    for (const Group& g : plan.groups)
        if (g.count)
            vg.push_back({&g.key, nullptr, g.count, (const uint8_t*)(inputs.data() + 5 * g.first), proofs.data() + upd::PROOF_BYTES * g.first,
                          verdict.data() + g.first});
    g16k_host_run(vg);
    for (uint64_t i = 0; i < n; ++i) ok[i] = (uint8_t)(bits[i] | ((plan.slot[i] != upd::NO_SLOT && verdict[plan.slot[i]]) ? BZK_UPD_PROOF : 0));
    if (aux_out) memcpy(aux_out, aux.data(), n * 32);
    if (commit_out) memcpy(commit_out, commit.data(), n * 32);
    return BZK_OK;
}

// ---- and on the device
int32_t run_device(bzk_ctx* ctx, const UpdParsed& P, const Plan& plan, const uint8_t state0[32], uint8_t* ok, uint8_t* aux_out, uint8_t* commit_out) {
    (void)hipSetDevice(ctx->device);
    const uint64_t n = P.rec.size();
    uint64_t cap_u = 1, cap_p = 1, cap_bytes = 1, cap_rows = 1, cap_nodes = 1;
    for (const Round& R : plan.rounds) {
        cap_u = std::max<uint64_t>(cap_u, R.mu());
        cap_p = std::max<uint64_t>(cap_p, R.row(0)[R.mu()]);
        cap_bytes = std::max<uint64_t>(cap_bytes, P.end(R.u1 - 1) - P.rec[R.u0].at);
        cap_rows = std::max<uint64_t>(cap_rows, R.rows.size());
        cap_nodes = std::max<uint64_t>(cap_nodes, R.n_nodes);
    }
    std::vector<G16kGroup> vg;   // the groups the verifier runs: a group whose key is refused keeps verdict 0
    for (const Group& g : plan.groups)
        if (g.count && g.key.valid) vg.push_back({&g.key, g.up.get(), g.count, nullptr, nullptr, nullptr});
    WsLayout ws("bzk_contract_updates_check");
    uint8_t *dbytes, *dsig, *dprev, *dbits, *dproofs, *dverdict, *dok;
    UpdRec* drec;
    PayRec* dpay;
    uint32_t *drows, *dslot;
    Fr *dnodes, *daux, *dcommit, *dinputs, *ddflt;
    G16kBufs vb;
    ws.take(dbytes, cap_bytes + 8); ws.take(drec, cap_u); ws.take(dpay, cap_p); ws.take(drows, cap_rows); ws.take(dnodes, cap_nodes);
    ws.take(dsig, cap_p); ws.take(dprev, (size_t)32 * plan.rounds.size()); ws.take(ddflt, plan.dflt.size());
    ws.take(daux, n); ws.take(dcommit, n); ws.take(dbits, n); ws.take(dslot, n); ws.take(dok, n);
    ws.take(dinputs, (size_t)5 * plan.n_slots + 1); ws.take(dproofs, (size_t)upd::PROOF_BYTES * plan.n_slots + 1); ws.take(dverdict, plan.n_slots + 1);
    if (!vg.empty()) g16k_declare(ws, vb, vg, false);
    BZK_TRY(ws.commit(ctx));
    {
        size_t v = 0;
        for (const Group& g : plan.groups)
            if (g.count && g.key.valid) {
                vg[v].inputs = (const uint8_t*)(dinputs + 5 * g.first);
                vg[v].proofs = dproofs + upd::PROOF_BYTES * g.first;
                vg[v++].ok = dverdict + g.first;
            }
    }
    upd::Consts c;
    const void* pc;
    BZK_TRY(poseidon_consts_dev_shared(ctx, 3, &pc, &c.rf3, &c.rp3));
    c.c3 = (const Fr29*)pc;
    BZK_TRY(poseidon_consts_dev_shared(ctx, 5, &pc, &c.rf5, &c.rp5));
    c.c5 = (const Fr29*)pc;
    BZK_TRY(poseidon_consts_dev_shared(ctx, 8, &pc, &c.rf8, &c.rp8));
    c.c8 = (const Fr29*)pc;
    c.dflt = ddflt;
    const uint32_t* tab = nullptr;
    if (!P.pay.empty()) BZK_TRY(ed25519_table_dev(ctx, &tab));
    BZK_HIP(ctx, hipMemcpyAsync(ddflt, plan.dflt.data(), plan.dflt.size() * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipMemcpyAsync(dslot, plan.slot.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    BZK_HIP(ctx, hipMemsetAsync(dverdict, 0, plan.n_slots + 1, ctx->stream));  // a group whose key is refused keeps verdict 0
    for (size_t r = 0; r < plan.rounds.size(); ++r) {  // one stream: a round's uploads follow the previous round's kernels
        const Round& R = plan.rounds[r];
        const UpdRec* rec = P.rec.data() + R.u0;
        const uint32_t mu = R.mu(), pay_base = rec[0].pay0, np = R.row(0)[mu], upd0 = (uint32_t)R.u0;
        const uint64_t base = rec[0].at;
        uint8_t* prev = dprev + 32 * r;
        BZK_HIP(ctx, hipMemcpyAsync(dbytes, P.bytes + base, P.end(R.u1 - 1) - base, hipMemcpyHostToDevice, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(drec, rec, (size_t)mu * sizeof(UpdRec), hipMemcpyHostToDevice, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(drows, R.rows.data(), R.rows.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        BZK_HIP(ctx, hipMemcpyAsync(prev, R.u0 ? P.bytes + P.rec[R.u0 - 1].at + P.rec[R.u0 - 1].next_off : state0, 32, hipMemcpyHostToDevice, ctx->stream));
        if (np) {
            bool deposits = false, withdraws = false;
            for (uint32_t t = 0; t < mu; ++t) {
                deposits |= rec[t].kind == upd::DEPOSIT && rec[t].pay_n;
                withdraws |= rec[t].kind == upd::WITHDRAW && rec[t].pay_n && rec[t].route;
            }
            BZK_HIP(ctx, hipMemcpyAsync(dpay, P.pay.data() + pay_base, (size_t)np * sizeof(PayRec), hipMemcpyHostToDevice, ctx->stream));
            if (deposits) {
                BZK_LAUNCH(ctx, "upd_deposit_sig", upd_deposit_sig_kernel, dim3((np + UPD_SIG_BLOCK - 1) / UPD_SIG_BLOCK), dim3(UPD_SIG_BLOCK), 0,
                           (const uint8_t*)dbytes, base, (const UpdRec*)drec, upd0, (const PayRec*)dpay, np, tab, dsig);
                BZK_LAUNCH(ctx, "upd_deposit_leaf", upd_deposit_leaf_kernel, dim3((np + UPD_HASH_BLOCK - 1) / UPD_HASH_BLOCK), dim3(UPD_HASH_BLOCK), 0,
                           (const uint8_t*)dbytes, base, (const UpdRec*)drec, upd0, (const PayRec*)dpay, np, c, dnodes);
            }
            if (withdraws)
                BZK_LAUNCH(ctx, "upd_withdraw_leaf", upd_withdraw_leaf_kernel, dim3((np + UPD_HASH_BLOCK - 1) / UPD_HASH_BLOCK), dim3(UPD_HASH_BLOCK), 0,
                           (const uint8_t*)dbytes, base, (const UpdRec*)drec, upd0, (const PayRec*)dpay, np, c, dnodes);
        }
        for (uint32_t k = 1; k <= R.depth; ++k) {
            const uint32_t lanes = R.row(k)[mu];
            if (!lanes) continue;
            BZK_LAUNCH(ctx, "upd_tree_level", upd_tree_level_kernel, dim3((lanes + UPD_HASH_BLOCK - 1) / UPD_HASH_BLOCK), dim3(UPD_HASH_BLOCK), 0,
                       dnodes, (const UpdRec*)drec, (const uint32_t*)(drows + (size_t)(k - 1) * (mu + 1)), (const uint32_t*)(drows + (size_t)k * (mu + 1)),
                       mu, R.level_at[k - 1], R.level_at[k], k, lanes, c);
        }
        BZK_LAUNCH(ctx, "upd_inputs", upd_inputs_kernel, dim3((mu + UPD_HASH_BLOCK - 1) / UPD_HASH_BLOCK), dim3(UPD_HASH_BLOCK), 0,
                   (const uint8_t*)dbytes, base, (const UpdRec*)drec, upd0, mu, (const uint8_t*)prev, (const Fr*)dnodes, (const uint8_t*)dsig, pay_base, c,
                   daux, dcommit, dbits, dinputs, dproofs);
    }
    BZK_TRY(g16k_enqueue(ctx, vb, vg, false, false));  // all live groups side by side: one set of launches per round
    BZK_LAUNCH(ctx, "upd_verdict", upd_verdict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (const uint32_t*)dslot, (const uint8_t*)dverdict,
               (const uint8_t*)dbits, n, dok);
    BZK_HIP(ctx, hipMemcpyAsync(ok, dok, n, hipMemcpyDeviceToHost, ctx->stream));
    if (aux_out) BZK_HIP(ctx, hipMemcpyAsync(aux_out, daux, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (commit_out) BZK_HIP(ctx, hipMemcpyAsync(commit_out, dcommit, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    BZK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the keys' upload buffers and the layout go out of scope after this
    return BZK_OK;
}

}  // namespace

int32_t contract_updates_run(bzk_ctx* ctx, const bzk_contract_desc& c, UpdParsed& P, const uint64_t* count, uint64_t m, uint64_t height0,
                             const uint8_t state0[32], uint8_t* ok, uint8_t* aux_out, uint8_t* commit_out) {
    Plan plan;
    make_plan(c, P, count, m, height0, plan);
    prepare_keys(plan, ctx != nullptr);
    if (ctx) return run_device(ctx, P, plan, state0, ok, aux_out, commit_out);
    return run_host(host_default_threads(), P, plan, state0, ok, aux_out, commit_out);
}

}  // namespace bzk
