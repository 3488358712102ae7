// CPU model of the MSM's partition front (bazuka_amd/csrc/msm_impl.cuh section 3d): the four passes - histogram, scan, scatter, bin pass - as plain loops
// over the very __host__ __device__ index functions the kernels use (msm_front.cuh), every array sized exactly as the call's workspace sizes it.  Built with
// -fsanitize=address,undefined and run as a program of its own (tests/test_msm_front_cpu.py): an index that would leave its array on the device aborts here.
// Checked per case: every non-zero digit lands exactly once inside its own bucket's [start, start + count), no index reaches len, count equals a direct
// histogram, iota / population keys are what msm_count wrote, and a forced tiny bin capacity takes the unstaged (chunked) path of the bin pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../bazuka_amd/csrc/msm_front.cuh"

using namespace bzk;

#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
            exit(1);                                            \
        }                                                       \
    } while (0)

struct Scalar { uint32_t l[8]; };

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static Scalar uniform() {
    Scalar s;
    for (int k = 0; k < 8; ++k) s.l[k] = rnd();
    s.l[7] &= 0x3fffffffu;  // < 2^254 < r
    return s;
}
// r - 1 (BLS12-381 scalar field), little-endian limbs
static const Scalar R_MINUS_1 = {{0x00000000u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}};
// every window's raw digit is v (windows that fit under bit 254)
static Scalar repeated_digit(int c, uint32_t v) {
    Scalar s = {};
    for (int w = 0; (w + 1) * c <= 254; ++w)
        for (int b = 0; b < c; ++b)
            if ((v >> b) & 1) s.l[(w * c + b) / 32] |= 1u << ((w * c + b) % 32);
    return s;
}
static const char* MIXES[] = {"uniform", "zero", "equal", "r-1", "carry", "small", "half-equal"};
static std::vector<Scalar> make(int mix, uint64_t n, int c) {
    std::vector<Scalar> v(n);
    const Scalar one = uniform();
    for (uint64_t i = 0; i < n; ++i) {
        switch (mix) {
            case 0: v[i] = uniform(); break;
            case 1: v[i] = Scalar{}; break;
            case 2: v[i] = one; break;
            case 3: v[i] = R_MINUS_1; break;
            case 4: v[i] = repeated_digit(c, (1u << (c - 1)) + (uint32_t)(i & 1)); break;  // 2^(c-1) and 2^(c-1) + 1: the carry boundary
            case 5: v[i] = Scalar{{rnd(), rnd() & 0xffffu, 0, 0, 0, 0, 0, 0}}; break;
            default: v[i] = i < n / 2 ? one : uniform(); break;
        }
    }
    return v;
}
static void excl_scan(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* total) {  // what front_block_excl_scan computes
    uint32_t run = 0;
    for (uint32_t k = 0; k < n; ++k) { const uint32_t x = in[k]; out[k] = run; run += x; }
    if (total) *total = run;
}

static uint64_t run_case(const std::vector<Scalar>& sc, int c, int w_begin, int wc, int w_total, uint32_t cap, const char* what) {
    const uint64_t n = sc.size();
    const FrontPlan P = msm_front_plan(n, n, c, wc, true, true, 2);
    CHECK(P.on, "%s: plan refuses n %llu c %d", what, (unsigned long long)n, c);
    const uint32_t half = 1u << (c - 1), nbins = P.nbins((uint32_t)wc), nb = (uint32_t)wc * half;
    const uint64_t len = (uint64_t)wc * n;
    CHECK(nbins % FRONT_SCAN_BINS == 0 && nbins <= (16u << FRONT_HI_MAX) && P.lo_bits <= FRONT_LO_MAX, "%s: shapes", what);
    // the workspace of the call, as msm_run declares it
    std::vector<uint32_t> tile_hist((size_t)P.n_tiles * nbins, 0xdeadbeefu), tile_off((size_t)P.n_tiles * nbins, 0xdeadbeefu), bin_total(nbins, 0xdeadbeefu),
        bin_base(nbins + 1, 0xdeadbeefu), inter(len, 0xffffffffu), vals_s(len, 0xffffffffu), start(nb, 0xdeadbeefu), count(nb, 0xdeadbeefu), iota(nb, 0xdeadbeefu),
        ckey(nb, 0xdeadbeefu);
    // 1. histogram
    for (uint32_t tile = 0; tile < P.n_tiles; ++tile) {
        std::vector<uint32_t> h(16u << FRONT_HI_MAX, 0);
        for (uint32_t j = 0; j < FRONT_TILE / FRONT_THREADS; ++j)
            for (uint32_t tid = 0; tid < FRONT_THREADS; ++tid) {
                const uint64_t i = (uint64_t)tile * FRONT_TILE + j * FRONT_THREADS + tid;
                if (i >= n) continue;
                msm_signed_digits(sc[i].l, c, w_total, [&](int w, uint32_t d, uint32_t) {
                    if (d && w >= w_begin && w < w_begin + wc) h.at(P.bin_of((uint32_t)(w - w_begin), d - 1))++;
                });
            }
        for (uint32_t b = 0; b < nbins; ++b) tile_hist.at(P.table_at(tile, b, nbins)) = h[b];
    }
    // 2. scan
    for (uint32_t blk = 0; blk < nbins / FRONT_SCAN_BINS; ++blk) {
        uint32_t sums[FRONT_SCAN_PARTS][FRONT_SCAN_BINS];
        for (uint32_t tid = 0; tid < FRONT_SCAN_BINS * FRONT_SCAN_PARTS; ++tid) {
            const uint32_t bl = tid % FRONT_SCAN_BINS, q = tid / FRONT_SCAN_BINS, b = blk * FRONT_SCAN_BINS + bl;
            uint32_t t0, t1, s = 0;
            front_scan_range(P.n_tiles, q, t0, t1);
            for (uint32_t t = t0; t < t1; ++t) s += tile_hist.at(P.table_at(t, b, nbins));
            sums[q][bl] = s;
        }
        for (uint32_t tid = 0; tid < FRONT_SCAN_BINS * FRONT_SCAN_PARTS; ++tid) {
            const uint32_t bl = tid % FRONT_SCAN_BINS, q = tid / FRONT_SCAN_BINS, b = blk * FRONT_SCAN_BINS + bl;
            uint32_t t0, t1, run = 0;
            front_scan_range(P.n_tiles, q, t0, t1);
            for (uint32_t k = 0; k < q; ++k) run += sums[k][bl];
            for (uint32_t t = t0; t < t1; ++t) {
                const uint32_t x = tile_hist.at(P.table_at(t, b, nbins));
                tile_off.at(P.table_at(t, b, nbins)) = run;
                run += x;
            }
            if (q == FRONT_SCAN_PARTS - 1) bin_total.at(b) = run;
        }
    }
    // 3. scatter
    constexpr uint32_t STAGE = FRONT_TILE * FRONT_GW, GB = FRONT_GW << FRONT_HI_MAX;
    for (uint32_t tile = 0; tile < P.n_tiles; ++tile) {
        std::vector<uint32_t> stage(STAGE, 0xffffffffu), bbase(16u << FRONT_HI_MAX), cnt_s(GB), tbs_s(GB), cur_s(GB), toff_s(GB);
        uint32_t total = 0;
        for (uint32_t b = 0; b < nbins; ++b) bbase.at(b) = bin_total.at(b);
        excl_scan(bbase.data(), bbase.data(), nbins, &total);
        if (tile == 0) {
            for (uint32_t b = 0; b < nbins; ++b) bin_base.at(b) = bbase[b];
            bin_base.at(nbins) = total;
        }
        for (uint32_t g0 = 0; g0 < (uint32_t)wc; g0 += FRONT_GW) {
            const uint32_t gw = std::min(FRONT_GW, (uint32_t)wc - g0), nbl = gw << P.hi_bits, b0 = g0 << P.hi_bits;
            for (uint32_t b = 0; b < nbl; ++b) {
                cnt_s.at(b) = tile_hist.at(P.table_at(tile, b0 + b, nbins));
                toff_s.at(b) = tile_off.at(P.table_at(tile, b0 + b, nbins));
            }
            excl_scan(cnt_s.data(), tbs_s.data(), nbl, nullptr);
            for (uint32_t b = 0; b < nbl; ++b) cur_s[b] = tbs_s[b];
            for (uint32_t j = 0; j < FRONT_TILE / FRONT_THREADS; ++j)
                for (uint32_t tid = 0; tid < FRONT_THREADS; ++tid) {
                    const uint64_t i = (uint64_t)tile * FRONT_TILE + j * FRONT_THREADS + tid;
                    if (i >= n) continue;
                    msm_signed_digits(sc[i].l, c, w_total, [&](int w, uint32_t d, uint32_t neg) {
                        const int lw = w - w_begin - (int)g0;
                        if (d && lw >= 0 && lw < (int)gw) {
                            const uint32_t pos = cur_s.at(P.bin_of((uint32_t)lw, d - 1))++;
                            CHECK(pos < STAGE, "%s: stage position %u", what, pos);
                            stage.at(pos) = P.pack((uint32_t)i, d - 1, neg);
                        }
                    });
                }
            for (uint32_t b = 0; b < nbl; ++b) {
                const uint32_t cn = cnt_s[b], src = tbs_s[b];
                const uint64_t dst = (uint64_t)bbase.at(b0 + b) + toff_s[b];
                CHECK(cur_s[b] == src + cn, "%s: tile %u bin %u ranked %u of %u", what, tile, b0 + b, cur_s[b] - src, cn);
                for (uint32_t e = 0; e < cn; ++e) {
                    CHECK(dst + e < len && src + e < STAGE, "%s: store %llu of %llu", what, (unsigned long long)(dst + e), (unsigned long long)len);
                    CHECK(inter.at(dst + e) == 0xffffffffu, "%s: intermediate slot written twice", what);
                    inter.at(dst + e) = stage.at(src + e);
                }
            }
        }
    }
    // 4. bin pass
    const uint32_t clamp = len / nb <= 64 ? 255u : 65535u;
    uint64_t unstaged = 0;
    for (uint32_t b = 0; b < nbins; ++b) {
        std::vector<uint32_t> stage(FRONT_BIN_CAP, 0xffffffffu), h(1u << FRONT_LO_MAX, 0), cur(1u << FRONT_LO_MAX, 0);
        const uint32_t nbu = 1u << P.lo_bits, lw = b >> P.hi_bits;
        uint32_t base, cnt;
        front_bin_range(bin_base.at(b), bin_base.at(b + 1), len, base, cnt);
        CHECK(cnt == bin_base[b + 1] - bin_base[b] && (cnt == 0 || base == bin_base[b]), "%s: bin %u taken as empty", what, b);
        const uint32_t g0 = P.first_bucket(b, half);
        CHECK((uint64_t)base + cnt <= len, "%s: bin %u ends at %llu", what, b, (unsigned long long)base + cnt);
        for (uint32_t e = 0; e < cnt; ++e) h.at(P.packed_lo(inter.at(base + e)))++;
        excl_scan(h.data(), cur.data(), nbu, nullptr);
        for (uint32_t k = 0; k < nbu; ++k) {
            const uint32_t g = g0 + k, cn = h[k];
            CHECK(g < nb, "%s: bucket %u of %u", what, g, nb);
            CHECK(start.at(g) == 0xdeadbeefu, "%s: bucket %u written twice", what, g);
            start.at(g) = base + cur[k];
            count.at(g) = cn;
            iota.at(g) = g;
            ckey.at(g) = front_pop_key(cn, clamp);
        }
        const bool staged = front_bin_staged(cnt, cap);
        if (!staged) ++unstaged;
        for (uint32_t e = 0; e < cnt; ++e) {
            const uint32_t v = inter.at(base + e);
            const uint32_t pos = cur.at(P.packed_lo(v))++;
            CHECK(pos < cnt, "%s: bin %u position %u of %u", what, b, pos, cnt);
            if (staged) stage.at(pos) = P.final_value(v, lw);
            else vals_s.at(base + pos) = P.final_value(v, lw);
        }
        if (staged)
            for (uint32_t e = 0; e < cnt; ++e) vals_s.at(base + e) = stage.at(e);
    }
    // ---- the properties
    std::vector<std::vector<uint32_t>> want(nb);
    uint64_t pairs = 0;
    for (uint64_t i = 0; i < n; ++i) {
        // the recoding checked on its own terms: sum of +-d_w 2^(c w) over all windows is the scalar (c w_total >= 256 and s < 2^255: no carry leaves the top)
        int64_t acc[12] = {};
        msm_signed_digits(sc[i].l, c, w_total, [&](int w, uint32_t d, uint32_t neg) {
            const int p = c * w;
            const uint64_t x = (uint64_t)d << (p % 32);
            acc[p / 32] += neg ? -(int64_t)(x & 0xffffffffu) : (int64_t)(x & 0xffffffffu);
            acc[p / 32 + 1] += neg ? -(int64_t)(x >> 32) : (int64_t)(x >> 32);
        });
        for (int k = 0; k < 11; ++k) {
            const int64_t carry = acc[k] >> 32;  // arithmetic shift: floor
            acc[k] -= carry * ((int64_t)1 << 32);
            acc[k + 1] += carry;
        }
        for (int k = 0; k < 12; ++k) CHECK(acc[k] == (k < 8 ? (int64_t)sc[i].l[k] : 0), "%s: the digits of scalar %llu do not add up to it (limb %d)", what, (unsigned long long)i, k);
        msm_signed_digits(sc[i].l, c, w_total, [&](int w, uint32_t d, uint32_t neg) {
            CHECK(d <= half, "%s: digit %u", what, d);
            if (d && w >= w_begin && w < w_begin + wc) {
                const uint32_t lw = (uint32_t)(w - w_begin);
                want.at(lw * half + d - 1).push_back((uint32_t)i | (lw << 27) | (neg << 31));
                ++pairs;
            }
        });
    }
    CHECK(bin_base[nbins] == pairs, "%s: %u pairs counted, %llu exist", what, bin_base[nbins], (unsigned long long)pairs);
    uint64_t at = 0;
    for (uint32_t g = 0; g < nb; ++g) {
        CHECK(count[g] == want[g].size(), "%s: bucket %u count %u, direct histogram %zu", what, g, count[g], want[g].size());
        CHECK(start[g] == at, "%s: bucket %u starts at %u, expected %llu", what, g, start[g], (unsigned long long)at);  // window-major, no gaps, no overlap
        CHECK((uint64_t)start[g] + count[g] <= len, "%s: bucket %u reaches %llu", what, g, (unsigned long long)start[g] + count[g]);
        CHECK(iota[g] == g && ckey[g] == std::min<uint32_t>(count[g], clamp), "%s: bucket %u iota / key", what, g);
        std::vector<uint32_t> got(vals_s.begin() + start[g], vals_s.begin() + start[g] + count[g]);
        std::sort(got.begin(), got.end());
        std::sort(want[g].begin(), want[g].end());
        CHECK(got == want[g], "%s: bucket %u holds other values than its digits", what, g);
        for (uint32_t v : got) CHECK((v & 0x07ffffffu) < n, "%s: value not clean under the mask", what);
        at += count[g];
    }
    return unstaged;
}

int main() {
    const uint64_t sizes[] = {1, 255, 4097, 70001};
    const int cs[] = {12, 13, 16};
    int cases = 0;
    for (int c : cs) {
        const int w_total = (256 + c - 1) / c;
        for (uint64_t n : sizes)
            for (int mix = 0; mix < 7; ++mix) {
                const std::vector<Scalar> sc = make(mix, n, c);
                char what[96];
                for (int wb = 0; wb < w_total; wb += 16) {  // the groups of <= 16 windows msm_run makes, then a split call's ranges
                    snprintf(what, sizeof what, "n %llu c %d %s windows [%d, %d)", (unsigned long long)n, c, MIXES[mix], wb, std::min(w_total, wb + 16));
                    run_case(sc, c, wb, std::min(16, w_total - wb), w_total, FRONT_BIN_CAP, what);
                    ++cases;
                }
                snprintf(what, sizeof what, "n %llu c %d %s windows [5, 10)", (unsigned long long)n, c, MIXES[mix]);
                run_case(sc, c, 5, 5, w_total, FRONT_BIN_CAP, what);
                // a bin capacity of one value: every fuller bin takes the unstaged path
                snprintf(what, sizeof what, "n %llu c %d %s tiny capacity", (unsigned long long)n, c, MIXES[mix]);
                const uint64_t unstaged = run_case(sc, c, 0, std::min(16, w_total), w_total, 1, what);
                CHECK(n < 255 || mix == 1 || unstaged > 0, "%s: the unstaged path was not taken", what);
                cases += 2;
            }
    }
    // an all-equal vector larger than the staging capacity with the real capacity: one bin per window holds everything
    {
        const std::vector<Scalar> sc = make(2, 20000, 16);
        CHECK(run_case(sc, 16, 0, 16, 16, FRONT_BIN_CAP, "n 20000 c 16 equal") > 0, "a 20000-value bin must exceed the staging capacity");
        ++cases;
    }
    // the plan itself: what must keep the sort, and the default's range
    CHECK(!msm_front_plan(1000, 1000, 16, 16, true, true, 1).on && !msm_front_plan(1000, 1000, 16, 16, false, true, 2).on, "plan: sort / ineligible");
    CHECK(!msm_front_plan(1000, 1000, 8, 16, true, true, 2).on && !msm_front_plan(1000, 1000, 18, 14, true, true, 2).on, "plan: window sizes outside [9, 17]");
    CHECK(!msm_front_plan(1u << 20, ((uint64_t)1 << 23) + 1, 16, 16, true, true, 2).on, "plan: index bits");
    CHECK(msm_front_plan(1u << 20, 1u << 20, 16, 16, true, true, 0).on && msm_front_plan(1u << 22, 1u << 22, 16, 16, true, true, 0).on, "plan: default on");
    CHECK(!msm_front_plan(1u << 20, 1u << 20, 16, 16, true, false, 0).on && !msm_front_plan(1u << 19, 1u << 19, 15, 15, true, true, 0).on &&
              !msm_front_plan(1u << 24, 1u << 24, 16, 16, true, true, 0).on && msm_front_plan(1u << 20, 1u << 20, 16, 16, true, false, 2).on,
          "plan: default off beside other work, at small window sizes and at 2^24 points");
    printf("msm_front_check ok: %d cases\n", cases);
    return 0;
}
