// Wire-form L1 transactions: what the parser (host_bincode.h parse_l1_txs) hands the kernels and the host entry points of eddsa.hip.  Plain C++:
// the per-lane code is bzk_l1.cuh's.
#pragma once
#include <stdint.h>

struct bzk_ctx;

namespace bzk {
namespace l1 {

constexpr uint32_t HAS_SRC = 1, SIGNED = 2;                // L1Rec::flags
constexpr uint64_t RECORD_MAX = (uint64_t)1 << 20;         // max_block_size (src/config/blockchain.rs:337): no block can carry a longer record
constexpr uint64_t CHUNK = (uint64_t)1 << 16;              // records staged per round of launches
constexpr uint64_t CHUNK_BYTES = (uint64_t)64 << 20;       // record bytes staged per round

// one parsed record; offsets are inside the record except `at`
struct L1Rec {
    uint32_t at;       // the record's first byte, from the staged bytes' first (set per round)
    uint32_t key_off;  // the 32 bytes of src (0 where src is None)
    uint32_t sig_off;  // the 64 signature bytes (0 where Unsigned)
    uint32_t sig_tag;  // the Signature enum's tag: the signed form ends here, followed by an Unsigned tag
    uint32_t cut_a;    // [cut_a, cut_b): the Option tag and payload of a Some(state) / Some(delta); cut_a == cut_b: none
    uint32_t cut_b;
    uint32_t flags;    // HAS_SRC | SIGNED
    uint32_t sig_tagv; // the Signature tag's value as read (0 Unsigned, 1 Signed)
};

}  // namespace l1

struct L1SoA {
    const uint8_t* txs;       // the records as received
    const uint64_t* rec_off;  // n + 1: where record i starts in txs
    const l1::L1Rec* rec;     // n (at unset)
};
// verdicts (ok, n bytes) and hashes (hash_out n x 32, may be null) of n parsed records on the device.  count non-null: the records are m
// block bodies, count[j] records each: root_out (m x 32) and sig_ok_out (m) are written too, from hashes that never left the device.  Synchronises.
int32_t l1_check_run(bzk_ctx* ctx, const L1SoA& t, uint64_t n, const uint64_t* count, uint64_t m, uint8_t* ok, uint8_t* hash_out,
                     uint8_t* sig_ok_out, uint8_t* root_out);
// the same on `threads` host threads
int32_t l1_check_host(int threads, const L1SoA& t, uint64_t n, const uint64_t* count, uint64_t m, uint8_t* ok, uint8_t* hash_out,
                      uint8_t* sig_ok_out, uint8_t* root_out);


}  // namespace bzk
