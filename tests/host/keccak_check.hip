// CPU harness of the device SHA3-256 (bazuka_amd/csrc/bzk_keccak.cuh): the same __host__ __device__ functions the gfx950 kernel runs per lane -
// sha3_256_one with its blanked range, and fr_from_le_bytes_mod - with the bound assertions of the field code on, called from
// tests/test_withdraw_admit_cpu.py through ctypes.
#define BZK_FP28_CHECK 1
#include <string.h>

#include "../../bazuka_amd/csrc/bzk_keccak.cuh"

using namespace bzk;

extern "C" {

// the layouts of bzk_sha3_256_batch; blank (n entries, may be null): the offset inside message i of the 32 bytes absorbed as zeros, or ~0 for none
int kc_sha3_batch(const uint8_t* data, const uint64_t* off, const uint64_t* blank, uint64_t n, uint8_t* digest_out, uint8_t* scalar_out) {
    for (uint64_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return -1;
        const uint64_t len = off[i + 1] - off[i];
        const uint64_t b = blank ? blank[i] : keccak::NO_BLANK;
        if (b != keccak::NO_BLANK && (b > len || len - b < keccak::BLANK_LEN)) return -1;
        const keccak::Digest d = keccak::sha3_256_one(data + off[i], len, b);
        if (digest_out) memcpy(digest_out + 32 * i, d.w, 32);
        if (scalar_out) {
            const Fe<FrParams> s = keccak::fr_from_le_bytes_mod(d);
            memcpy(scalar_out + 32 * i, s.l, 32);
        }
    }
    return 0;
}

// out[i] = ZkScalar::new of the 32 little-endian bytes in[i], Montgomery limbs
int kc_scalar_new_batch(const uint8_t* in, uint64_t n, uint8_t* out) {
    for (uint64_t i = 0; i < n; ++i) {
        keccak::Digest d;
        memcpy(d.w, in + 32 * i, 32);
        const Fe<FrParams> s = keccak::fr_from_le_bytes_mod(d);
        memcpy(out + 32 * i, s.l, 32);
    }
    return 0;
}
}
