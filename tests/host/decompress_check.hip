// CPU harness of the key decompression's device code (bazuka_amd/csrc/bzk_decompress.cuh): the same __host__ __device__ functions the gfx950
// kernels run per lane - the Fr square root, decompress_one, and the per-transaction composition decompress -> hash input -> Poseidon ->
// verify_one - with the bound assertions of the 29-bit field on, called from tests/test_decompress_cpu.py through ctypes.
#define BZK_FP28_CHECK 1
#include <string.h>

#include <vector>

#include "../../bazuka_amd/csrc/bzk_decompress.cuh"
#include "../../bazuka_amd/csrc/bzk_poseidon_opt.h"

using namespace bzk;

namespace {
// the sparse Poseidon constants of width t from the reference's plain layout (rc then mds, 8 x 32-bit Montgomery), as the library derives them
bool sparse_consts(int t, const uint8_t* consts, int n_consts, int rf, int rp, std::vector<Fr29>& c) {
    if (n_consts != (rf + rp) * t + t * t) return false;
    std::vector<Fr> rc((size_t)(rf + rp) * t), mds((size_t)t * t), flat;
    for (size_t i = 0; i < rc.size(); ++i) memcpy(rc[i].l, consts + 32 * i, 32);
    for (size_t i = 0; i < mds.size(); ++i) memcpy(mds[i].l, consts + 32 * (rc.size() + i), 32);
    if (!poseidon_optimize(t, rf, rp, rc, mds, flat)) return false;
    c.resize(flat.size());
    for (size_t i = 0; i < flat.size(); ++i) c[i] = fr29::norm(fr29::to29(flat[i]));
    return true;
}
}  // namespace

extern "C" {

// out[i] = a square root of in[i] (Montgomery limbs of residues' limbs), ok[i] = 1; or ok[i] = 0 for a non-residue
int dc_sqrt_batch(const uint8_t* in, uint64_t n, uint8_t* out, uint8_t* ok) {
    for (uint64_t i = 0; i < n; ++i) {
        Fr a;
        memcpy(&a, in + 32 * i, 32);
        if (!eddsa::canonical(a)) return -1;
        bool res;
        const Fr s = fr29::from29(eddsa::f29_sqrt(fr29::to29(a), &res));
        memcpy(out + 32 * i, &s, 32);
        ok[i] = res ? 1 : 0;
    }
    return 0;
}

// the layouts of bzk_jubjub_decompress_batch
int dc_decompress_batch(const uint8_t* x, const uint8_t* odd, uint64_t n, uint8_t* xy_out, uint8_t* ok) {
    for (uint64_t i = 0; i < n; ++i) {
        Fr xi, o[2];
        memcpy(&xi, x + 32 * i, 32);
        ok[i] = eddsa::decompress_one(xi, odd[i] != 0, o);
        memcpy(xy_out + 64 * i, o, 64);
    }
    return 0;
}

// n parsed transactions in the arrays the device path stages: src_x, dst_x n x 32; src_odd, dst_odd n bytes; tok n x 64 (amount token id | fee token
// id); nums n x 3 u64 (nonce, amount, fee); sig n x 96.  consts8 / consts6: the Poseidon constants of widths 8 and 6.  ok: n verdicts, hash: n x 32.
int dc_tx_verify(const uint8_t* src_x, const uint8_t* src_odd, const uint8_t* dst_x, const uint8_t* dst_odd, const uint8_t* tok, const uint64_t* nums,
                 const uint8_t* sig, uint64_t n, const uint8_t* consts8, int n_consts8, const uint8_t* consts6, int n_consts6, int rf, int rp,
                 uint8_t* ok, uint8_t* hash) {
    std::vector<Fr29> c8, c6, tab;
    if (!sparse_consts(8, consts8, n_consts8, rf, rp, c8) || !sparse_consts(6, consts6, n_consts6, rf, rp, c6)) return -2;
    eddsa::base_table_build(tab);
    for (uint64_t i = 0; i < n; ++i) {
        Fr sx, dx, src[2], dst[2], tk[2], s[3], tuple[7];
        memcpy(&sx, src_x + 32 * i, 32);
        memcpy(&dx, dst_x + 32 * i, 32);
        memcpy(tk, tok + 64 * i, 64);
        memcpy(s, sig + 96 * i, 96);
        const uint8_t sok = eddsa::decompress_one(sx, src_odd[i] != 0, src), dok = eddsa::decompress_one(dx, dst_odd[i] != 0, dst);
        const bool tok_ok = eddsa::tx_tuple_one(nums + 3 * i, tk, dst, dok, tuple);
        const Fr h = tok_ok ? poseidon29_hash<8>(tuple, c8.data(), rf, rp) : Fr::zero();
        uint32_t lane[eddsa::TAB_WORDS];
        const uint8_t v = eddsa::verify_one(src, &h, s, c6.data(), rf, rp, tab.data(), lane, 1);
        ok[i] = (v && sok && tok_ok) ? 1 : 0;
        memcpy(hash + 32 * i, &h, 32);
    }
    return 0;
}
}
