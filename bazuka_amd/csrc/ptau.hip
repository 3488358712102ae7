// The powers-of-tau accumulator (phase 1 of a ceremony): bzk_ptau_size, bzk_ptau_init, bzk_ptau_contribute, bzk_ptau_check.  Host code only: the
// points of a contribution go through pmul.hip's powers form (five calls), the sums of a check through the MSMs (or host threads without a context),
// the subgroup checks through subgroup.hip, the pairing products through rekey.hip's pairings_equal.
//   blob = "BZKPTAU1" | u32 log_m | u32 0 | tau_g1[2m - 1] | tau_g2[m] | alpha_g1[m] | beta_g1[m] | beta_g2,  m = 2^log_m, raw records
#include <stddef.h>
#include <string.h>

#include <vector>

#include "bzk_internal.h"
#include "bzk_pmul.h"
#include "bzk_subgroup.cuh"
#include "host_zk.h"

namespace bzk {
namespace {

constexpr char MAGIC[9] = "BZKPTAU1";
constexpr uint64_t HEADER = 16;
enum Arr { A_HEADER = 0, A_TAU_G1 = 1, A_TAU_G2 = 2, A_ALPHA_G1 = 3, A_BETA_G1 = 4, A_BETA_G2 = 5, A_KEY = 6 };

struct Shape {
    uint32_t log_m = 0;
    uint64_t m = 0;
    uint64_t off[6] = {0, 0, 0, 0, 0, 0};  // by array code; off[0] unused
    uint64_t cnt[6] = {0, 0, 0, 0, 0, 0};
    uint64_t size = 0;
};
bool shape_of(uint32_t log_m, Shape& s) {
    if (log_m < 1 || log_m > 24) return false;
    s.log_m = log_m;
    s.m = (uint64_t)1 << log_m;
    const uint64_t cnt[6] = {0, 2 * s.m - 1, s.m, s.m, s.m, 1};
    uint64_t at = HEADER;
    for (int a = 1; a < 6; ++a) {
        s.off[a] = at;
        s.cnt[a] = cnt[a];
        at += cnt[a] * (a == A_TAU_G2 || a == A_BETA_G2 ? 192 : 96);
    }
    s.size = at;
    return true;
}
bool parse(const uint8_t* blob, uint64_t len, Shape& s) {
    uint32_t w[2];
    if (!blob || len < HEADER || memcmp(blob, MAGIC, 8) != 0) return false;
    memcpy(w, blob + 8, 8);
    return w[1] == 0 && shape_of(w[0], s) && s.size == len;
}
bool is_g2(int a) { return a == A_TAU_G2 || a == A_BETA_G2; }

void g1_raw(const hp::G1A& p, uint8_t out[96]) {
    memcpy(out, p.x.l, 48);
    memcpy(out + 48, p.y.l, 48);
}
void g2_raw(const hp::G2A& p, uint8_t out[192]) {
    memcpy(out, p.x.c0.l, 48);
    memcpy(out + 48, p.x.c1.l, 48);
    memcpy(out + 96, p.y.c0.l, 48);
    memcpy(out + 144, p.y.c1.l, 48);
}
// a raw record that passed the subgroup check (finite, in range, on the curve) as a pairing operand
hp::G1A g1_of(const uint8_t* raw) {
    hp::G1A p;
    memcpy(p.x.l, raw, 48);
    memcpy(p.y.l, raw + 48, 48);
    p.inf = false;
    return p;
}
hp::G2A g2_of(const uint8_t* raw) {
    uint8_t packed[193];
    memcpy(packed, raw, 192);
    packed[192] = 0;
    hp::G2A p;
    (void)hp::g2_unpack(packed, p);
    return p;
}
bool fr_ok_nonzero(const uint8_t* k) {
    Fr a;
    memcpy(a.l, k, 32);
    bool below = false;
    for (int i = 7; i >= 0; --i)
        if (a.l[i] != FrParams::MOD[i]) {
            below = a.l[i] < FrParams::MOD[i];
            break;
        }
    return below && !a.is_zero();
}

// S0 = sum_i rho_i q[i], S1 = sum_i rho_i q[i + 1] over i < n (q holds n + 1 records): device MSMs with a context, host sums without
template <class F, class PtA>
int32_t shifted_sums(bzk_ctx* ctx, bool g2, const uint8_t* q, uint64_t n, const uint8_t seed[32], uint8_t code, PtA& s0, PtA& s1) {
    const size_t sz = g2 ? 192 : 96;
    if (!ctx) {
        AffineT<F> a0, a1;
        s0.inf = !host_seeded_sum<F>(q, n, seed, code, a0);
        s1.inf = !host_seeded_sum<F>(q + sz, n, seed, code, a1);
        memcpy(&s0.x, &a0, sizeof a0);
        memcpy(&s1.x, &a1, sizeof a1);
        return BZK_OK;
    }
    std::vector<uint8_t> rho(32 * n);
    host_for_each(n, host_default_threads(), [&](uint64_t i) { rho_of(seed, code, i, rho.data() + 32 * i); });
    uint8_t p0[193], p1[193];
    if (g2) {
        BZK_TRY(bzk_msm_g2(ctx, q, rho.data(), n, BZK_F_CANONICAL, p0));
        BZK_TRY(bzk_msm_g2(ctx, q + sz, rho.data(), n, BZK_F_CANONICAL, p1));
    } else {
        BZK_TRY(bzk_msm_g1(ctx, q, rho.data(), n, BZK_F_CANONICAL, p0));
        BZK_TRY(bzk_msm_g1(ctx, q + sz, rho.data(), n, BZK_F_CANONICAL, p1));
    }
    s0.inf = p0[sz] != 0;
    s1.inf = p1[sz] != 0;
    memcpy(&s0.x, p0, sz);
    memcpy(&s1.x, p1, sz);
    return BZK_OK;
}
static_assert(offsetof(hp::G1A, y) == 48 && offsetof(hp::G2A, y) == 96, "a pairing operand starts with the raw record");

int32_t fail(uint64_t report[4], uint64_t array, uint64_t index, uint64_t code) {
    report[0] = array;
    report[1] = index;
    report[2] = code;
    report[3] = 0;
    return 0;
}

}  // namespace
}  // namespace bzk

using namespace bzk;

extern "C" {

uint64_t bzk_ptau_size(uint32_t log_m) {
    Shape s;
    return shape_of(log_m, s) ? s.size : 0;
}

int32_t bzk_ptau_init(uint32_t log_m, uint8_t* out, uint64_t cap) {
    Shape s;
    if (!out || !shape_of(log_m, s) || cap < s.size) return BZK_E_ARG;
    uint8_t g1[96], g2[192];
    g1_raw(g1_gen(), g1);
    g2_raw(g2_gen(), g2);
    const uint32_t head[2] = {log_m, 0};
    memcpy(out, MAGIC, 8);
    memcpy(out + 8, head, 8);
    for (int a = 1; a < 6; ++a)
        for (uint64_t i = 0; i < s.cnt[a]; ++i) {
            if (is_g2(a)) memcpy(out + s.off[a] + 192 * i, g2, 192);
            else memcpy(out + s.off[a] + 96 * i, g1, 96);
        }
    return BZK_OK;
}

int32_t bzk_ptau_contribute(bzk_ctx* ctx, const uint8_t* in, uint64_t len, const uint8_t secrets[96], uint8_t* out, uint64_t cap, uint8_t key_out[576]) {
    Shape s;
    if (!in || !secrets || !out || !key_out || !parse(in, len, s) || cap < s.size) return BZK_E_ARG;
    const uint8_t *tau = secrets, *alpha = secrets + 32, *beta = secrets + 64;
    if (!fr_ok_nonzero(tau) || !fr_ok_nonzero(alpha) || !fr_ok_nonzero(beta)) return BZK_E_ARG;
    const Fr one_fr = Fr::one();
    const uint8_t* one = (const uint8_t*)one_fr.l;
    // the key and beta_g2 on the host: one-point calls of the same function
    uint8_t g2[192], key[576], beta_g2[192];
    g2_raw(g2_gen(), g2);
    for (int k = 0; k < 3; ++k) {
        PmCall c;
        c.g2 = true;
        c.pts = g2;
        c.n = 1;
        c.c = secrets + 32 * k;
        c.s = one;
        c.out = key + 192 * k;
        BZK_TRY(pm_run(nullptr, "bzk_ptau_contribute", c));
    }
    {
        PmCall c;
        c.g2 = true;
        c.pts = in + s.off[A_BETA_G2];
        c.n = 1;
        c.c = beta;
        c.s = one;
        c.out = beta_g2;
        BZK_TRY(pm_run(nullptr, "bzk_ptau_contribute", c));
    }
    if (out != in) memcpy(out, in, HEADER);
    const uint8_t* lead[5] = {nullptr, one, one, alpha, beta};
    for (int a = A_TAU_G1; a <= A_BETA_G1; ++a) {
        PmCall c;
        c.g2 = is_g2(a);
        c.pts = in + s.off[a];
        c.n = s.cnt[a];
        c.c = lead[a];
        c.s = tau;
        c.out = out + s.off[a];
        BZK_TRY(pm_run(ctx, "bzk_ptau_contribute", c));
    }
    memcpy(out + s.off[A_BETA_G2], beta_g2, 192);
    memcpy(key_out, key, 576);
    return BZK_OK;
}

int32_t bzk_ptau_check(bzk_ctx* ctx, const uint8_t* before, uint64_t before_len, const uint8_t key[576], const uint8_t* after, uint64_t after_len,
                       const uint8_t seed[32], uint64_t report[4]) {
    if (!after || !seed || !report || (before == nullptr) != (key == nullptr)) return BZK_E_ARG;
    memset(report, 0, 32);
    Shape s, sb;
    if (!parse(after, after_len, s)) return fail(report, A_HEADER, 0, 0);
    if (before && (!parse(before, before_len, sb) || sb.log_m != s.log_m)) return fail(report, A_HEADER, 1, 0);
    // every point of the order-r subgroup; a record that is no finite curve point (the identity's zero bytes among them) has verdict 2
    for (int a = 1; a < 6; ++a) {
        uint64_t idx = 0;
        uint8_t code = 0;
        BZK_TRY(sg_first_bad(ctx, "bzk_ptau_check", is_g2(a), after + s.off[a], false, s.cnt[a], &idx, &code));
        if (idx != s.cnt[a]) return fail(report, a, idx, code);
    }
    uint8_t g1b[96], g2b[192];
    const hp::G1A G1 = g1_gen();
    const hp::G2A G2 = g2_gen();
    g1_raw(G1, g1b);
    g2_raw(G2, g2b);
    if (memcmp(after + s.off[A_TAU_G1], g1b, 96) != 0) return fail(report, A_TAU_G1, 0, 0);
    if (memcmp(after + s.off[A_TAU_G2], g2b, 192) != 0) return fail(report, A_TAU_G2, 0, 0);
    const hp::G2A tau2 = g2_of(after + s.off[A_TAU_G2] + 192);
    const hp::G1A tau1 = g1_of(after + s.off[A_TAU_G1] + 96);
    // consecutive entries differ by one factor tau: e(S1, G2) == e(S0, tau_g2[1]) on the G1 arrays, e(tau_g1[1], T0) == e(G1, T1) on tau_g2
    for (int a = A_TAU_G1; a <= A_BETA_G1; ++a) {
        const uint64_t n = s.cnt[a] - 1;
        if (is_g2(a)) {
            hp::G2A t0, t1;
            BZK_TRY((shifted_sums<HFp2Ops>(ctx, true, after + s.off[a], n, seed, (uint8_t)a, t0, t1)));
            if (t0.inf || t1.inf || !pairings_equal(tau1, t0, G1, t1)) return fail(report, a, 0, 0);
        } else {
            hp::G1A s0, s1;
            BZK_TRY((shifted_sums<HFpOps>(ctx, false, after + s.off[a], n, seed, (uint8_t)a, s0, s1)));
            if (s0.inf || s1.inf || !pairings_equal(s1, G2, s0, tau2)) return fail(report, a, 0, 0);
        }
    }
    if (!pairings_equal(g1_of(after + s.off[A_BETA_G1]), G2, G1, g2_of(after + s.off[A_BETA_G2]))) return fail(report, A_BETA_G2, 0, 0);
    if (before) {
        // after = before times the key's exponents: tau on tau_g1[1], alpha on alpha_g1[0], beta on beta_g1[0]
        const uint64_t at[3] = {s.off[A_TAU_G1] + 96, s.off[A_ALPHA_G1], s.off[A_BETA_G1]};
        for (int k = 0; k < 3; ++k) {
            const uint8_t v = sg_host_one(true, key + 192 * k);
            if (v != sg::IN_SUBGROUP) return fail(report, A_KEY, k, v);
            uint8_t packed[97];
            memcpy(packed, before + at[k], 96);
            packed[96] = 0;
            hp::G1A b;
            if (!hp::g1_unpack(packed, b)) return fail(report, A_KEY, k, sg::INVALID);
            if (!pairings_equal(g1_of(after + at[k]), G2, b, g2_of(key + 192 * k))) return fail(report, A_KEY, k, 0);
        }
    }
    return 1;
}

}  // extern "C"
