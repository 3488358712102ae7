// Wire-form MpnTransaction / MpnWithdraw / MpnDeposit records: what the parsers (host_bincode.h parse_txs, parse_withdraws, parse_deposits) hand
// the device orchestration and the host entry points of eddsa.hip.  Plain C++: the per-lane code is bzk_eddsa.cuh's, bzk_decompress.cuh's,
// bzk_keccak.cuh's and bzk_ed25519.cuh's.
#pragma once
#include <stdint.h>

struct bzk_ctx;

namespace bzk {

// n parsed MpnTransactions as the arrays the device stages (host memory; parse_txs fills them from bincode without any field arithmetic)
struct TxSoA {
    const uint8_t *src_x, *dst_x;      // n x 32: PointCompressed.0
    const uint8_t *src_odd, *dst_odd;  // n: PointCompressed.1
    const uint8_t* tok;                // n x 64: amount token id | fee token id as scalars
    const uint64_t* nums;              // n x 3: nonce, amount, fee
    const uint8_t* sig;                // n x 96: r.x | r.y | s
};
constexpr uint64_t MPN_TX_CHUNK = (uint64_t)1 << 16;  // transactions staged per round of launches: where the signature kernel's rate has levelled off
// eddsa.hip: MpnTransaction::verify_signature for each; ok n bytes; hash_out n x 32, src_xy_out / dst_xy_out n x 64 (the decompressed keys) or null;
// synchronises
int32_t mpn_tx_verify_run(bzk_ctx* ctx, const TxSoA& t, uint64_t n, uint8_t* ok, uint8_t* hash_out, uint8_t* src_xy_out, uint8_t* dst_xy_out);
// n parsed MpnWithdraws (host memory; parse_withdraws cuts them out of the bincode without hashing or field arithmetic)
struct WdSoA {
    const uint8_t* txs;        // the records as received
    const uint64_t* rec_off;   // n + 1: where record i starts in txs
    const uint64_t* pay_off;   // n: where its ContractWithdraw starts in txs
    const uint32_t* pay_len;   // n: the payment's length
    const uint32_t* cd_off;    // n: calldata's offset inside the payment
    const uint8_t* key_x;      // n x 32: PointCompressed.0
    const uint8_t* key_odd;    // n: PointCompressed.1
    const uint32_t* nonce;     // n
    const uint8_t* sig;        // n x 96: r.x | r.y | s
};
constexpr uint64_t MPN_WD_PAYMENT_MAX = (uint64_t)1 << 16;    // a longer ContractWithdraw is refused as malformed (its memo is unbounded on the wire)
constexpr uint64_t MPN_WD_CHUNK_BYTES = (uint64_t)64 << 20;   // payment bytes staged per round of launches
// eddsa.hip: ok n bytes (bit 0 verify_signature, bit 1 verify_calldata); fp_out n x 32 (payment.fingerprint()), xy_out n x 64 (the decompressed
// keys) or null; synchronises
int32_t mpn_withdraw_verify_run(bzk_ctx* ctx, const WdSoA& t, uint64_t n, uint8_t* ok, uint8_t* fp_out, uint8_t* xy_out);
// n parsed MpnDeposits (host memory; parse_deposits cuts them out of the bincode without hashing or field arithmetic)
struct DpSoA {
    const uint8_t* txs;        // the records as received
    const uint64_t* rec_off;   // n + 1: where record i starts in txs
    const uint64_t* pay_off;   // n: where its ContractDeposit starts in txs
    const uint32_t* tag_off;   // n: the Option<Signature> tag's offset inside the payment: the signed bytes are payment[0 .. tag_off) | 0x00
    const uint32_t* src_off;   // n: the 32 bytes of payment.src, offset inside the payment
    const uint32_t* sig_off;   // n: the 64 signature bytes, offset inside the payment (0 where sig is None)
    const uint8_t* has_sig;    // n: 1 / 0
    const uint8_t* key_x;      // n x 32: PointCompressed.0
    const uint8_t* key_odd;    // n: PointCompressed.1
};
// eddsa.hip: ok n bytes (bit 0 payment.verify_signature(), bit 1 mpn_address decompresses); xy_out n x 64 (the decompressed addresses) or null;
// chunked like mpn_withdraw_verify_run; synchronises
int32_t mpn_deposit_verify_run(bzk_ctx* ctx, const DpSoA& t, uint64_t n, uint8_t* ok, uint8_t* xy_out);
// eddsa.hip: the same per-lane Ed25519 code on the host, for record i
uint8_t mpn_deposit_sig_host(const DpSoA& t, uint64_t i);

}  // namespace bzk
