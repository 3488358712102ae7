// CPU harness of the signature verifier's device code (bazuka_amd/csrc/bzk_eddsa.cuh verify_one): the same __host__ __device__ function the gfx950
// kernel runs per lane, with the bound assertions of the 29-bit field on, called from tests/test_eddsa_cpu.py through ctypes.
#define BZK_FP28_CHECK 1
#include <string.h>

#include <vector>

#include "../../bazuka_amd/csrc/bzk_eddsa.cuh"
#include "../../bazuka_amd/csrc/bzk_poseidon_opt.h"

using namespace bzk;

extern "C" {

// ok[i] = verdict of entry i.  pub_xy: n x 64, msg: n x 32, sig: n x 96 (the layouts of bzk_jubjub_verify_batch).  consts = the Poseidon
// constants of width 6, rc then mds in the reference's plain layout (8 x 32-bit Montgomery, n_consts entries): the sparse form is derived here
// as the library derives it.
int ec_verify_batch(const uint8_t* pub_xy, const uint8_t* msg, const uint8_t* sig, uint64_t n, const uint8_t* consts, int n_consts, int rf, int rp,
                    uint8_t* ok) {
    constexpr int T = 6;
    if (n_consts != (rf + rp) * T + T * T) return -2;
    std::vector<Fr> rc((size_t)(rf + rp) * T), mds((size_t)T * T), flat;
    for (size_t i = 0; i < rc.size(); ++i) memcpy(rc[i].l, consts + 32 * i, 32);
    for (size_t i = 0; i < mds.size(); ++i) memcpy(mds[i].l, consts + 32 * (rc.size() + i), 32);
    if (!poseidon_optimize(T, rf, rp, rc, mds, flat)) return -3;
    std::vector<Fr29> c(flat.size()), tab;
    for (size_t i = 0; i < flat.size(); ++i) c[i] = fr29::norm(fr29::to29(flat[i]));
    eddsa::base_table_build(tab);
    for (uint64_t i = 0; i < n; ++i) {
        Fr p[2], m, s[3];
        memcpy(p, pub_xy + 64 * i, 64);
        memcpy(&m, msg + 32 * i, 32);
        memcpy(s, sig + 96 * i, 96);
        uint32_t lane[eddsa::TAB_WORDS];
        ok[i] = eddsa::verify_one(p, &m, s, c.data(), rf, rp, tab.data(), lane, 1);
    }
    return 0;
}
}
