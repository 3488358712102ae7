// CPU harness of the device SHA-512 and Ed25519 (bazuka_amd/csrc/bzk_sha512.cuh, bzk_ed25519.cuh): the same __host__ __device__ functions the
// gfx950 kernels run per lane - sha512_one over its byte ranges, sc_reduce512, the field 2^255 - 19, key decoding, verify_one - with the bound
// assertions on, called from tests/test_ed25519_cpu.py through ctypes.
#define BZK_FP28_CHECK 1
#include <string.h>

#include "../../bazuka_amd/csrc/bzk_ed25519.cuh"

using namespace bzk;

extern "C" {

// SHA-512 of p0[0 .. l0) | p1[0 .. l1) | p2[0 .. l2) | (tail >= 0: that byte)
int ed_sha512_ranges(const uint8_t* p0, uint64_t l0, const uint8_t* p1, uint64_t l1, const uint8_t* p2, uint64_t l2, int32_t tail, uint8_t out[64]) {
    sha512::Msg m;
    m.p[0] = p0; m.len[0] = l0;
    m.p[1] = p1; m.len[1] = l1;
    m.p[2] = p2; m.len[2] = l2;
    m.tail = tail;
    const sha512::Digest d = sha512::sha512_one(m);
    memcpy(out, d.w, 64);
    return 0;
}

// out = the 64 little-endian bytes in[i] mod l
int ed_sc_reduce_batch(const uint8_t* in, uint64_t n, uint8_t* out) {
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t x[16], r[8];
        memcpy(x, in + 64 * i, 64);
        ed25519::sc_reduce512(x, r);
        memcpy(out + 32 * i, r, 32);
    }
    return 0;
}

// field operations on 32-byte little-endian values below 2^255 (not necessarily below p); canonical bytes out.
// op: 0 a b, 1 a^2, 2 1 / a, 3 a^((p - 5) / 8), 4 a + b, 5 a - b
int ed_fe_op(int op, const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) {
    uint32_t aw[8], bw[8], ow[8];
    memcpy(aw, a, 32);
    memcpy(bw, b, 32);
    const ed25519::Fe x = ed25519::fe_from_words(aw), y = ed25519::fe_from_words(bw);
    ed25519::Fe r;
    switch (op) {
        case 0: r = ed25519::fe_mul(x, y); break;
        case 1: r = ed25519::fe_sq(x); break;
        case 2: r = ed25519::fe_invert(x); break;
        case 3: r = ed25519::fe_pow22523(x); break;
        case 4: r = ed25519::fe_add(x, y); break;
        case 5: r = ed25519::fe_sub(x, y); break;
        default: return -1;
    }
    ed25519::fe_to_words(r, ow);
    memcpy(out, ow, 32);
    return 0;
}

// 1 / 0: the key decodes; xy_out = x | y as canonical bytes
int ed_decode(const uint8_t key[32], uint8_t xy_out[64]) {
    uint32_t kw[8], w[8];
    memcpy(kw, key, 32);
    ed25519::Fe x, y;
    const bool ok = ed25519::decode(kw, x, y);
    ed25519::fe_to_words(x, w);
    memcpy(xy_out, w, 32);
    ed25519::fe_to_words(y, w);
    memcpy(xy_out + 32, w, 32);
    return ok ? 1 : 0;
}

// 1 / 0: the message is msg[0 .. len) followed by the byte `tail` where tail >= 0
int ed_verify(const uint8_t pk[32], const uint8_t* msg, uint64_t len, int32_t tail, const uint8_t sig[64]) {
    sha512::Msg body = sha512::msg_one(msg, len);
    body.tail = tail;
    return ed25519::verify_host(pk, sig, body);
}
}
