// Wire-form ContractUpdates: the per-lane code of updates.hip's kernels.  __host__ __device__: the ctx = NULL entry runs the same functions on host
// threads.  What `update_contract` computes per update before it looks at the proof:
//
//   commit            ZkScalar::new(sha3(bincode((prover, reward))))       src/blockchain/ops/apply_tx/update_contract/mod.rs:29-32
//   aux, Deposit      root of List{capacity, Struct{1, token, amount, calldata}}                                 deposit.rs:16-55
//   aux, Withdraw     root of List{capacity, Struct{1, token, amount, fee token, fee, fingerprint, calldata}}    withdraw.rs:16-72
//   aux, FunctionCall H2(token, fee)                                                                             function_call.rs:28-44
//   ContractDeposit::verify_signature  Ed25519 over the payment with sig := None                          src/core/transaction.rs:192-202
//   ContractWithdraw::fingerprint      ZkScalar::new(sha3(bincode(payment with calldata := 0)))                  :204-211
//
// A list's root is the 4-ary Poseidon tree over its item hashes; an item that was never set hashes as zeros, and a subtree without a set item
// is the level's default (ZkStateBuilder::compress, src/zk/state.rs).
#pragma once
#include "bzk_ed25519.cuh"
#include "bzk_keccak.cuh"
#include "bzk_l1.cuh"
#include "bzk_poseidon29.cuh"
#include "bzk_updates.h"

namespace bzk {
namespace upd {

// the Poseidon constants of arity 2, 4 and 7 (widths 3, 5, 8) and the default nodes d[w][k]: w = 0 for four-field items, 1 for seven-field ones
struct Consts {
    const Fr29 *c3, *c5, *c8;
    int rf3, rp3, rf5, rp5, rf8, rp8;
    const Fr* dflt;  // 2 x (MAX_CAPACITY + 1)
};
BZK_HD const Fr& default_node(const Consts& c, uint32_t kind, uint32_t level) { return c.dflt[(kind == WITHDRAW ? MAX_CAPACITY + 1 : 0) + level]; }

BZK_HD uint32_t rd32(const uint8_t* p) {  // any alignment
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
BZK_HD uint64_t rd64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
BZK_HD Fr fr_load(const uint8_t* p) {  // the 32 bytes of a ZkScalar as they lie on the wire: Montgomery limbs
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = rd32(p + 4 * i);
    return r;
}
BZK_HD Fr fr_from_u64(uint64_t v) {  // ZkScalar::from(u64)
    Fr c = Fr::zero();
    c.l[0] = (uint32_t)v;
    c.l[1] = (uint32_t)(v >> 32);
    return fe_to_mont<FrParams>(c);
}
// Money { token_id: ContractId, amount } at p: the token's scalar (`impl From<ContractId> for ZkScalar`: Null 0, Ziesha 1, Custom its scalar)
// and the amount in Montgomery form
BZK_HD void money_one(const uint8_t* p, Fr& token, Fr& amount) {
    const uint32_t tag = rd32(p);
    token = tag == 1 ? Fr::one() : Fr::zero();
    if (tag == 2) token = fr_load(p + 4);
    amount = fr_from_u64(rd64(p + (tag == 2 ? 36 : 4)));
}

// the item hash of deposit p: H4(1, token, amount, calldata)
BZK_HD Fr deposit_leaf(const uint8_t* pay, const PayRec& p, const Consts& c) {
    Fr in[4];
    in[0] = Fr::one();
    money_one(pay + p.amt_off, in[1], in[2]);
    in[3] = fr_load(pay + p.cd_off);
    return poseidon29_hash<5>(in, c.c5, c.rf5, c.rp5);
}
// the item hash of withdrawal p: H7(1, token, amount, fee token, fee, fingerprint, calldata)
BZK_HD Fr withdraw_leaf(const uint8_t* pay, const PayRec& p, const Consts& c) {
    Fr in[7];
    in[0] = Fr::one();
    money_one(pay + p.amt_off, in[1], in[2]);
    money_one(pay + p.fee_off, in[3], in[4]);
    in[5] = keccak::fr_from_le_bytes_mod(keccak::sha3_256_one(pay, p.len, p.cd_off));
    in[6] = fr_load(pay + p.cd_off);
    return poseidon29_hash<8>(in, c.c8, c.rf8, c.rp8);
}
// ContractDeposit::verify_signature: None does not verify; else Ed25519 over payment[0 .. tag_off) | 00
BZK_HD uint8_t deposit_sig(const uint8_t* pay, const PayRec& p, const uint32_t* __restrict__ base_tab, uint32_t* lane, int stride) {
    if (!(p.flags & PAY_HAS_SIG)) return 0;
    sha512::Msg body = sha512::msg_one(pay, p.tag_off);
    body.tail = 0;  // the None tag of the unsigned form
    return ed25519::verify_one(pay + p.src_off, pay + p.sig_off, body, base_tab, lane, stride);
}

// ---- the trees of a round.  Row k of `rows` (mu + 1 prefix sums) says how many nodes every update of the round has at level k: row 0 its
// payments, row k = ceil(row k - 1 / 4) up to its function's capacity, nothing above it and nothing for an update without ROUTE.  Level k's nodes
// of all updates lie together from level_at[k] in the round's node array.
// parent j (a lane of level k >= 1): H4 of children 4 j .. 4 j + 3 of level k - 1, a child beyond the update's count being that level's default
BZK_HD void tree_parent_one(Fr* nodes, const UpdRec* __restrict__ rec, const uint32_t* __restrict__ below, const uint32_t* __restrict__ row,
                            uint32_t mu, uint32_t below_at, uint32_t row_at, uint32_t k, uint32_t lane, const Consts& c) {
    const uint32_t u = l1::tree_of(row, mu, lane), j = lane - row[u];
    const uint32_t have = below[u + 1] - below[u];
    const Fr* child = nodes + (size_t)below_at + below[u];
    const Fr d = default_node(c, rec[u].kind, k - 1);
    Fr in[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        in[q] = d;
        if (4 * j + q < have) in[q] = child[4 * j + q];
    }
    nodes[(size_t)row_at + row[u] + j] = poseidon29_hash<5>(in, c.c5, c.rf5, c.rp5);
}

// ---- one update's proof inputs: (commit, height, prev state, aux, next_state) as 5 x 32 Montgomery bytes.  rec: the update's record; prev: the
// 32 bytes of the state the update is checked against (state0, or the next_state.state_hash its predecessor claims).  Returns aux (zeros without
// ROUTE or for a Mint) and the commitment; writes the inputs and the proof into the key group's arrays where the update has a slot.
BZK_HD void inputs_one(const uint8_t* rec, const UpdRec& u, const uint8_t* prev, const Fr* nodes, const Consts& c, Fr& aux, Fr& commit, Fr* inputs,
                       uint8_t* proofs) {
    commit = keccak::fr_from_le_bytes_mod(keccak::sha3_256_one(rec + u.commit_off, 48, keccak::NO_BLANK));
    aux = Fr::zero();
    if (u.route) {
        if (u.kind == CALL) {
            Fr in[2];
            money_one(rec + u.data_off, in[0], in[1]);
            aux = poseidon29_hash<3>(in, c.c3, c.rf3, c.rp3);
        } else if (u.kind != MINT) {
            aux = u.root == NO_SLOT ? default_node(c, u.kind, u.capacity) : nodes[u.root];
        }
    }
    if (u.slot == NO_SLOT) return;
    Fr* in = inputs + (size_t)5 * u.slot;
    in[0] = commit;
    in[1] = fr_from_u64(u.height);
    in[2] = fr_load(prev);
    in[3] = aux;
    in[4] = fr_load(rec + u.next_off);
    uint8_t* pr = proofs + (size_t)PROOF_BYTES * u.slot;  // neither side is aligned: 96 words moved as words of any alignment, then 3 bytes
    const uint8_t* src = rec + u.proof_off;
#pragma unroll 4
    for (uint32_t i = 0; i < PROOF_BYTES / 4; ++i) {
        const uint32_t w = rd32(src + 4 * i);
        __builtin_memcpy(pr + 4 * i, &w, 4);
    }
    for (uint32_t i = PROOF_BYTES / 4 * 4; i < PROOF_BYTES; ++i) pr[i] = src[i];
}
// SIGS: every deposit of the update verified (1 for the other kinds); sig: the verdicts of the call's payments
BZK_HD uint8_t sigs_all(const UpdRec& u, const uint8_t* __restrict__ sig) {
    uint8_t all = 1;
    if (u.kind == DEPOSIT)
        for (uint32_t i = 0; i < u.pay_n; ++i) all &= sig[i] ? 1 : 0;
    return all;
}

}  // namespace upd
}  // namespace bzk
