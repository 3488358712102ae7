// n points times one scalar (bzk_g1_scale_batch[_dev]) and what a Groth16 re-key is made of: bzk_params_rekey on a resident key, and the host
// arithmetic behind bzk_bellman_params_rekey[_check] (host_bellman.hip): the two deltas times d, the seeded sums and the pairing products.
// The per-point arithmetic and the recoding of the scalar are bzk_scale.cuh's scale_point and recode; this file holds the kernel, the rounds and the
// entry points.  No lane waits for another (no LDS, no barrier), and no step of a lane depends on its point: the digit string is the launch's.
#include <string.h>

#include <vector>

#include "bzk_internal.h"
#include "bzk_pmul.h"
#include "bzk_rekey.h"
#include "bzk_scale.cuh"
#include "bzk_stage.h"
#include "bzk_subgroup_host.h"
#include "host_pairing.h"
#include "host_threads.h"
#include "host_zk.h"

namespace bzk {
namespace {

constexpr int SC_BLOCK = 64;
constexpr uint64_t SC_ROUND = (uint64_t)1 << 18;      // points per staged round of a host-pointer call (subgroup.hip's)
constexpr uint64_t SC_DEV_ROUND = (uint64_t)1 << 24;  // points per launch over device-resident records

// out may be pts (a lane has read its record before it writes): neither is __restrict__
__global__ void __launch_bounds__(SC_BLOCK) g1_scale_kernel(const uint32_t* pts, uint32_t n, const uint32_t* __restrict__ dig, uint32_t* out,
                                                            uint8_t* inf) {
    const uint32_t i = blockIdx.x * SC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t v = sc::scale_point<sc::ScFp28>(pts + (size_t)24 * i, dig, out + (size_t)24 * i);
    if (inf) inf[i] = v;
}

bool fr_below_r(const Fr& a) {
    for (int i = 7; i >= 0; --i)
        if (a.l[i] != FrParams::MOD[i]) return a.l[i] < FrParams::MOD[i];
    return false;
}
bool fr_is_zero(const Fr& a) {
    uint32_t o = 0;
    for (int i = 0; i < 8; ++i) o |= a.l[i];
    return o == 0;
}

void host_run(const uint8_t* pts, uint64_t n, const sc::Digits& dg, uint8_t* out, uint8_t* inf) {
    host_for_each(n, host_default_threads(), [&](uint64_t i) {
        uint32_t w[24], o[24];
        memcpy(w, pts + 96 * i, 96);
        const uint8_t v = sc::scale_point<SgHFp>(w, dg.w, o);
        memcpy(out + 96 * i, o, 96);
        if (inf) inf[i] = v;
    });
}

// the rounds of one call.  Host records go up and come back through one staging buffer per round (the kernel runs in place); records in device
// memory are read and written where they lie.  The digit string is one more buffer of the call's layout, uploaded before the first launch and on
// the wipe list
int32_t run_rounds(bzk_ctx* ctx, const char* who, const uint8_t* pts, bool on_device, uint64_t n, const sc::Digits& dg, uint8_t* out, uint8_t* inf) {
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, who, n, on_device ? SC_DEV_ROUND : SC_ROUND);
    uint8_t *dp = nullptr, *di = nullptr, *ddig = nullptr;
    if (!on_device) {
        st.in(dp, pts, 96);
        st.out_part(dp, out, 96, 0);
        st.out(di, inf, 1);
    }
    st.ws.take(ddig, sizeof dg);
    st.wipe(ddig, sizeof dg);
    BZK_TRY(st.ws.commit(ctx));
    return st.run([&](uint64_t a, uint64_t m) {
        if (a == 0) BZK_TRY(st.dev.up(ddig, &dg, sizeof dg));
        const uint32_t* src = (const uint32_t*)(on_device ? pts + 96 * a : dp);
        uint32_t* dst = (uint32_t*)(on_device ? out + 96 * a : dp);
        uint8_t* flags = on_device ? (inf ? inf + a : nullptr) : di;
        BZK_LAUNCH(ctx, "g1_scale", g1_scale_kernel, dim3((unsigned)((m + SC_BLOCK - 1) / SC_BLOCK)), dim3(SC_BLOCK), 0, src, (uint32_t)m,
                   (const uint32_t*)ddig, dst, flags);
        return BZK_OK;
    });
}

Fp fp_hex(const char* hex) {  // 96 hex digits, big-endian, canonical -> Montgomery
    Fp c = Fp::zero();
    for (int i = 0; i < 96; ++i) {
        const char ch = hex[i];
        const uint32_t v = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
        const int nib = 95 - i;
        c.l[nib / 8] |= v << ((nib % 8) * 4);
    }
    return fe_to_mont<FpParams>(c);
}

}  // namespace

// shared with ptau.hip (bzk_pmul.h)
hp::G1A g1_gen() {
    return {hp::to_h(fp_hex("17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")),
            hp::to_h(fp_hex("08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")), false};
}
hp::G2A g2_gen() {
    return {{hp::to_h(fp_hex("024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")),
             hp::to_h(fp_hex("13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"))},
            {hp::to_h(fp_hex("0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801")),
             hp::to_h(fp_hex("0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be"))},
            false};
}
// e(a, q1) == e(b, q2), as one product e(a, q1) e(-b, q2) that must be one
bool pairings_equal(const hp::G1A& a, const hp::G2A& q1, const hp::G1A& b, const hp::G2A& q2) {
    hp::G1A p[2] = {a, b};
    p[1].y = HFpOps::neg(p[1].y);
    const hp::G2A q[2] = {q1, q2};
    bool degenerate = false;
    const hp::E12 f = hp::multi_miller(p, q, 2, &degenerate);
    return !degenerate && hp::e12_is_one(hp::final_exp(f));
}

void rho_of(const uint8_t seed[32], uint8_t code, uint64_t i, uint8_t out32[32]) {  // the low 16 bytes of the digest, as a canonical 32-byte integer
    uint8_t msg[41], h[32];
    memcpy(msg, seed, 32);
    msg[32] = code;
    memcpy(msg + 33, &i, 8);  // little-endian host
    sha3_256(msg, sizeof msg, h);
    memcpy(out32, h, 16);
    memset(out32 + 16, 0, 16);
}

namespace {

// S = sum_i rho_i q_i on host threads (bzk_pmul.h host_seeded_sum)
hp::G1A host_sum(const uint8_t* q, uint64_t n, const uint8_t seed[32], uint8_t code) {
    AffineT<HFpOps> a;
    hp::G1A r;
    r.inf = !host_seeded_sum<HFpOps>(q, n, seed, code, a);
    r.x = a.x;
    r.y = a.y;
    return r;
}

}  // namespace

int32_t g1_scale_run(bzk_ctx* ctx, const char* who, const uint8_t* pts, bool on_device, uint64_t n, const uint8_t k[32], uint8_t* out, uint8_t* inf) {
    Fr km;
    memcpy(km.l, k, 32);
    if (!fr_below_r(km)) return BZK_E_ARG;
    if (n == 0) return BZK_OK;
    sc::Digits dg;
    sc::recode(km, dg);
    wipe_host(&km, sizeof km);
    int32_t st = BZK_OK;
    if (!ctx) host_run(pts, n, dg, out, inf);
    else st = run_rounds(ctx, who, pts, on_device, n, dg, out, inf);
    wipe_host(&dg, sizeof dg);
    return st;
}

int32_t rekey_scalars(const uint8_t d[32], uint8_t dinv[32]) {
    Fr dm;
    memcpy(dm.l, d, 32);
    if (!fr_below_r(dm) || fr_is_zero(dm)) return BZK_E_ARG;
    Fr di = fe_inv<FrParams>(dm);
    memcpy(dinv, di.l, 32);
    wipe_host(&dm, sizeof dm);
    wipe_host(&di, sizeof di);
    return BZK_OK;
}

void rekey_vk_head(uint8_t vk870[870], const uint8_t d[32]) {
    if (!vk870[580 + 96]) {  // delta_g1: the batch function on one point
        uint8_t inf = 0;
        (void)g1_scale_run(nullptr, "rekey_vk_head", vk870 + 580, false, 1, d, vk870 + 580, &inf);
    }
    if (!vk870[677 + 192]) {  // delta_g2
        Fr dm;
        memcpy(dm.l, d, 32);
        Fr dc = fe_from_mont<FrParams>(dm);
        AffineT<HFp2Ops> p, a;
        memcpy(&p, vk870 + 677, 192);
        xyzz_to_affine<HFp2Ops>(host_mul<HFp2Ops>(p, dc.l, 256), a);  // d != 0 and delta_g2 of order r: finite
        memcpy(vk870 + 677, &a, 192);
        wipe_host(&dm, sizeof dm);
        wipe_host(&dc, sizeof dc);
    }
}

bool rekey_delta_consistent(const uint8_t vk870[870]) {
    hp::G1A d1;
    hp::G2A d2;
    if (!hp::g1_unpack(vk870 + 580, d1) || !hp::g2_unpack(vk870 + 677, d2)) return false;
    return pairings_equal(d1, g2_gen(), g1_gen(), d2);
}

int32_t rekey_ratio(bzk_ctx* ctx, uint8_t code, const uint8_t* before, const uint8_t* after, uint64_t n, const uint8_t seed[32],
                    const uint8_t vk_before[870], const uint8_t vk_after[870], bool* holds) {
    *holds = false;
    hp::G2A q0, q1;
    if (!hp::g2_unpack(vk_before + 677, q0) || !hp::g2_unpack(vk_after + 677, q1)) return BZK_OK;
    hp::G1A s0, s1;
    if (n == 0) {
        *holds = true;
        return BZK_OK;
    }
    if (!ctx) {
        s0 = host_sum(before, n, seed, code);
        s1 = host_sum(after, n, seed, code);
    } else {
        std::vector<uint8_t> rho(32 * n);
        host_for_each(n, host_default_threads(), [&](uint64_t i) { rho_of(seed, code, i, rho.data() + 32 * i); });
        uint8_t p0[97], p1[97];
        BZK_TRY(bzk_msm_g1(ctx, before, rho.data(), n, BZK_F_CANONICAL, p0));
        BZK_TRY(bzk_msm_g1(ctx, after, rho.data(), n, BZK_F_CANONICAL, p1));
        if (!hp::g1_unpack(p0, s0) || !hp::g1_unpack(p1, s1)) return BZK_E_INTERNAL;
    }
    *holds = pairings_equal(s1, q1, s0, q0);
    return BZK_OK;
}

}  // namespace bzk

using namespace bzk;

extern "C" {

int32_t bzk_g1_scale_batch(bzk_ctx* ctx, const uint8_t* pts, uint64_t n, const uint8_t k[32], uint8_t* out, uint8_t* inf_out) {
    if (!k || (n && (!pts || !out))) return BZK_E_ARG;
    return g1_scale_run(ctx, "bzk_g1_scale_batch", pts, false, n, k, out, inf_out);
}
int32_t bzk_g1_scale_batch_dev(bzk_ctx* ctx, const void* pts_dev, uint64_t n, const uint8_t k[32], void* out_dev, void* inf_out_dev) {
    if (!ctx || !k || (n && (!pts_dev || !out_dev))) return BZK_E_ARG;
    if (((uintptr_t)pts_dev | (uintptr_t)out_dev) & 3) return BZK_E_ARG;  // the records are read and written as 32-bit words
    return g1_scale_run(ctx, "bzk_g1_scale_batch_dev", (const uint8_t*)pts_dev, true, n, k, (uint8_t*)out_dev, (uint8_t*)inf_out_dev);
}

int32_t bzk_params_rekey(bzk_ctx* ctx, const bzk_params* params, const uint8_t d[32], bzk_params** out, uint8_t vk870_out[870]) {
    if (!ctx || !params || !d || !out) return BZK_E_ARG;
    *out = nullptr;
    uint8_t dinv[32];
    BZK_TRY(rekey_scalars(d, dinv));
    bzk_params* p = nullptr;
    void* dev[5];
    const void* src[5];
    uint64_t cnt[5];
    int32_t st = params_clone_shape(ctx, params, &p, dev, src, cnt);
    if (st == BZK_OK) {
        const size_t sz[5] = {96, 96, 96, 96, 192};
        for (int k = 2; k < 5 && st == BZK_OK; ++k)  // a, b_g1, b_g2 do not change
            if (cnt[k] && hipMemcpyAsync(dev[k], src[k], cnt[k] * sz[k], hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
                ctx->last_error = "bzk_params_rekey: device copy of a query";
                st = BZK_E_DEVICE;
            }
        for (int k = 0; k < 2 && st == BZK_OK; ++k)  // h, l times d^-1 (the call synchronises: the copies above are done with it)
            st = g1_scale_run(ctx, "bzk_params_rekey", (const uint8_t*)src[k], true, cnt[k], dinv, (uint8_t*)dev[k], nullptr);
        if (st == BZK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = BZK_E_DEVICE;
    }
    wipe_host(dinv, sizeof dinv);
    if (st != BZK_OK) {
        if (p) bzk_params_free(ctx, p);
        return st;
    }
    uint8_t vk[870];
    uint64_t got = 0;
    (void)bzk_params_read(ctx, p, 0, vk, 870, &got);  // the clone's head is the source's
    rekey_vk_head(vk, d);
    bzk_params_set_vk_internal(p, vk);
    if (vk870_out) memcpy(vk870_out, vk, 870);
    *out = p;
    return BZK_OK;
}

}  // extern "C"
