// Ed25519 signing of wire-form records: what ed_sign.hip offers wire.hip's entry points (bzk_mpn_deposits_sign, bzk_l1_txs_sign).  Plain C++: the
// per-lane code is bzk_ed25519_sign.cuh's.
#pragma once
#include <stdint.h>

#include "bzk_l1.h"
#include "bzk_mpn_wire.h"

struct bzk_ctx;

namespace bzk {

constexpr uint64_t ED25519_SIGN_ROUND = (uint64_t)1 << 16;        // rows (records) a host-pointer call stages per round
constexpr uint64_t ED25519_SIGN_ROUND_BYTES = (uint64_t)64 << 20; // message (record) bytes staged per round

// ContractDeposit signing for n parsed MpnDeposits and n keys (n x 64: secret | public): sig n x 64, ok n.  ok[i] = 1 where payment.src is the
// key's public half; else 0 and a zero sig row.  On the device when ctx is set (rounds of ED25519_SIGN_ROUND records or ED25519_SIGN_ROUND_BYTES;
// synchronises; the staged and expanded keys are overwritten), else the same per-lane code on `threads` host threads.
int32_t mpn_deposits_sign_all(bzk_ctx* ctx, int threads, const DpSoA& t, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* ok);
// The same for n parsed L1 records; ok[i] = 0 also where src is None.  hash_out (n x 32, may be null): Transaction::hash of every record.
int32_t l1_txs_sign_all(bzk_ctx* ctx, int threads, const L1SoA& t, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* ok, uint8_t* hash_out);

}  // namespace bzk
