// Wire-form ContractUpdates: what the parser (host_bincode.h parse_contract_updates) hands the kernels and the host path of updates.hip.  Plain
// C++: the per-lane code is bzk_updates.cuh's.
#pragma once
#include <stdint.h>

namespace bzk {
namespace upd {

constexpr uint32_t DEPOSIT = 0, WITHDRAW = 1, CALL = 2, MINT = 3;          // ContractUpdateData's variant index (UpdRec::kind)
constexpr uint32_t PAY_HAS_SIG = 1, PAY_CONTRACT = 2, PAY_CIRCUIT = 4;    // PayRec::flags: sig is Some; contract_id / circuit id are the update's
constexpr uint32_t NO_SLOT = 0xffffffffu;                                  // UpdRec::slot of an update that joins no key group
constexpr uint64_t RECORD_MAX = (uint64_t)1 << 20;        // max_block_size (src/config/blockchain.rs:337): no transaction can carry a longer update
constexpr uint64_t ROUND_PAYMENTS = (uint64_t)1 << 16;    // payments staged per round of launches (an update is never split)
constexpr uint64_t ROUND_BYTES = (uint64_t)64 << 20;      // record bytes staged per round
constexpr uint32_t MAX_CAPACITY = 8;                      // log4_payment_capacity above this is refused: 4^8 payments exceed any record
constexpr uint32_t PROOF_BYTES = 387, INPUT_BYTES = 5 * 32;

// one parsed update; offsets are inside the record except `at`
struct UpdRec {
    uint64_t at;          // the record's first byte in the call's `updates`
    uint64_t height;      // set by the call: height0 + the index of the update's transaction
    uint32_t kind;        // DEPOSIT .. MINT
    uint32_t circuit_id;
    uint32_t pay0;        // its payments: [pay0, pay0 + pay_n) of the call's PayRec array (none for CALL / MINT)
    uint32_t pay_n;
    uint32_t data_off;    // CALL: the fee (Money); MINT: the amount; else the payments' length word
    uint32_t next_off;    // next_state.state_hash (32 bytes)
    uint32_t commit_off;  // u64 32 | prover | u64 reward: 48 contiguous bytes that ARE bincode((prover, reward))
    uint32_t proof_off;   // the 387 bytes of the Groth16Proof
    // set by the call from its function table and the round's tree plan (no bytes of the record are read for these)
    uint32_t slot;        // its position in the key groups' arrays, NO_SLOT where ROUTE is clear or the update is a Mint
    uint32_t capacity;    // log4_payment_capacity of its function (0 for CALL)
    uint32_t route;       // 1: ROUTE holds
    uint32_t root;        // the node of the round's node array that is its payments' root (NO_SLOT: no payments, or no tree)
};
// one parsed payment; offsets are inside the payment except `off`
struct PayRec {
    uint32_t upd;      // its update (index in the call)
    uint32_t off;      // the payment's first byte inside its update's record
    uint32_t len;
    uint32_t slot;     // i: the payment's index in its update
    uint32_t cd_off;   // calldata (32 bytes)
    uint32_t amt_off;  // amount: Money (ContractId tag [| 32 bytes] | u64)
    uint32_t fee_off;  // fee: Money
    uint32_t tag_off;  // deposit: the Option<Signature> tag; the signed form is payment[0 .. tag_off) | 00
    uint32_t src_off;  // deposit: the 32 key bytes
    uint32_t sig_off;  // deposit: the 64 signature bytes (0 where sig is None)
    uint32_t flags;    // PAY_*
    uint32_t pad;
};

}  // namespace upd
}  // namespace bzk
