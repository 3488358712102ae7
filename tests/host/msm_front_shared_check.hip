// CPU model of the partition front's SHARED form (bazuka_amd/csrc/msm_impl.cuh section 3d, FrontPlan::shared): the levels of a full window table feed one
// bucket set - the four passes as plain loops over the very __host__ __device__ index functions the kernels use (msm_front.cuh), every array sized exactly
// as the call's workspace sizes it.  Built with -fsanitize=address,undefined and run as a program of its own (tests/test_msm_front_shared_cpu.py): an index
// that would leave its array on the device aborts here.  Checked per case: every non-zero digit of every requested level lands exactly once inside its own
// bucket's [start, start + count) as table index | sign, bins are contiguous and in key order, count equals a direct histogram, iota / population keys are
// what msm_count wrote, a prefix of the set gathers with the set's stride, and a forced tiny bin capacity takes the unstaged path of the bin pass.
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
static const char* MIXES[] = {"uniform", "zero", "equal", "r-1", "carry", "small", "half-equal", "one-bucket"};
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
            case 6: v[i] = i < n / 2 ? one : uniform(); break;
            default: v[i] = repeated_digit(c, 5); break;  // the same digit in every window of every scalar: all the call's pairs in ONE bucket
        }
    }
    return v;
}
static void excl_scan(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* total) {  // what front_block_excl_scan computes
    uint32_t run = 0;
    for (uint32_t k = 0; k < n; ++k) { const uint32_t x = in[k]; out[k] = run; run += x; }
    if (total) *total = run;
}

// levels [w_begin, w_begin + wc) of a table of w_total levels x table_n points, the first sc.size() points of it
static uint64_t run_case(const std::vector<Scalar>& sc, int c, int w_begin, int wc, int w_total, uint64_t table_n, uint32_t cap, const char* what) {
    const uint64_t n = sc.size();
    const FrontPlan P = msm_front_plan(n, (uint64_t)w_total * table_n, c, wc, true, true, 2, table_n);
    CHECK(P.on && P.shared, "%s: plan refuses n %llu c %d", what, (unsigned long long)n, c);
    const uint32_t half = 1u << (c - 1), nbins = P.shared_bins(), ntab = P.shared_tab(), nb = half;
    const uint64_t len = (uint64_t)wc * n;
    CHECK(ntab % FRONT_SCAN_BINS == 0 && ntab <= FRONT_SHARED_TAB_MAX && nbins <= (1u << FRONT_SHARED_HI_MAX) && P.lo_bits <= FRONT_LO_MAX &&
              P.hi_bits + P.lo_bits == (uint32_t)c - 1 && P.groups * FRONT_GW_SHARED >= (uint32_t)wc, "%s: shapes", what);
    // the workspace of the call, as msm_run declares it
    std::vector<uint32_t> tile_hist((size_t)P.n_tiles * ntab, 0xdeadbeefu), tile_off((size_t)P.n_tiles * ntab, 0xdeadbeefu), bin_total(ntab, 0xdeadbeefu),
        bin_base(ntab + 1, 0xdeadbeefu), vals_s(len, 0xffffffffu), start(nb, 0xdeadbeefu), count(nb, 0xdeadbeefu), iota(nb, 0xdeadbeefu), ckey(nb, 0xdeadbeefu);
    std::vector<uint64_t> inter(len, ~0ull);
    // 1. histogram
    for (uint32_t tile = 0; tile < P.n_tiles; ++tile) {
        std::vector<uint32_t> h(FRONT_SHARED_TAB_MAX, 0);
        for (uint32_t j = 0; j < FRONT_TILE / FRONT_THREADS; ++j)
            for (uint32_t tid = 0; tid < FRONT_THREADS; ++tid) {
                const uint64_t i = (uint64_t)tile * FRONT_TILE + j * FRONT_THREADS + tid;
                if (i >= n) continue;
                msm_signed_digits(sc[i].l, c, w_total, [&](int w, uint32_t d, uint32_t) {
                    if (d && w >= w_begin && w < w_begin + wc) h.at(P.shared_entry(P.shared_bin(d - 1), P.shared_group((uint32_t)(w - w_begin))))++;
                });
            }
        for (uint32_t b = 0; b < ntab; ++b) tile_hist.at(P.table_at(tile, b, ntab)) = h[b];
    }
    // 2. scan (the plain form's kernel, over the entries)
    for (uint32_t blk = 0; blk < ntab / FRONT_SCAN_BINS; ++blk) {
        uint32_t sums[FRONT_SCAN_PARTS][FRONT_SCAN_BINS];
        for (uint32_t tid = 0; tid < FRONT_SCAN_BINS * FRONT_SCAN_PARTS; ++tid) {
            const uint32_t bl = tid % FRONT_SCAN_BINS, q = tid / FRONT_SCAN_BINS, b = blk * FRONT_SCAN_BINS + bl;
            uint32_t t0, t1, s = 0;
            front_scan_range(P.n_tiles, q, t0, t1);
            for (uint32_t t = t0; t < t1; ++t) s += tile_hist.at(P.table_at(t, b, ntab));
            sums[q][bl] = s;
        }
        for (uint32_t tid = 0; tid < FRONT_SCAN_BINS * FRONT_SCAN_PARTS; ++tid) {
            const uint32_t bl = tid % FRONT_SCAN_BINS, q = tid / FRONT_SCAN_BINS, b = blk * FRONT_SCAN_BINS + bl;
            uint32_t t0, t1, run = 0;
            front_scan_range(P.n_tiles, q, t0, t1);
            for (uint32_t k = 0; k < q; ++k) run += sums[k][bl];
            for (uint32_t t = t0; t < t1; ++t) {
                const uint32_t x = tile_hist.at(P.table_at(t, b, ntab));
                tile_off.at(P.table_at(t, b, ntab)) = run;
                run += x;
            }
            if (q == FRONT_SCAN_PARTS - 1) bin_total.at(b) = run;
        }
    }
    // 3. scatter
    constexpr uint32_t STAGE = FRONT_TILE * FRONT_GW_SHARED, GB = 1u << FRONT_SHARED_HI_MAX;
    for (uint32_t tile = 0; tile < P.n_tiles; ++tile) {
        std::vector<uint64_t> stage(STAGE, ~0ull);
        std::vector<uint32_t> bbase(FRONT_SHARED_TAB_MAX), cnt_s(GB), tbs_s(GB), cur_s(GB), toff_s(GB);
        uint32_t total = 0;
        for (uint32_t b = 0; b < ntab; ++b) bbase.at(b) = bin_total.at(b);
        excl_scan(bbase.data(), bbase.data(), ntab, &total);
        if (tile == 0) {
            for (uint32_t b = 0; b < ntab; ++b) bin_base.at(b) = bbase[b];
            bin_base.at(ntab) = total;
        }
        for (uint32_t g0 = 0; g0 < (uint32_t)wc; g0 += FRONT_GW_SHARED) {
            const uint32_t gw = std::min(FRONT_GW_SHARED, (uint32_t)wc - g0), nbl = P.shared_bins();
            auto entry = [&](uint32_t b) { return P.shared_entry(b, P.shared_group(g0)); };
            for (uint32_t b = 0; b < nbl; ++b) {
                cnt_s.at(b) = tile_hist.at(P.table_at(tile, entry(b), ntab));
                toff_s.at(b) = tile_off.at(P.table_at(tile, entry(b), ntab));
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
                            const uint32_t pos = cur_s.at(P.shared_bin(d - 1))++;
                            CHECK(pos < STAGE, "%s: stage position %u", what, pos);
                            stage.at(pos) = P.shared_pack((uint32_t)w, (uint32_t)i, d - 1, neg);
                        }
                    });
                }
            for (uint32_t b = 0; b < nbl; ++b) {
                const uint32_t cn = cnt_s[b], src = tbs_s[b];
                const uint64_t dst = (uint64_t)bbase.at(entry(b)) + toff_s[b];
                CHECK(cur_s[b] == src + cn, "%s: tile %u bin %u ranked %u of %u", what, tile, b, cur_s[b] - src, cn);
                for (uint32_t e = 0; e < cn; ++e) {
                    CHECK(dst + e < len && src + e < STAGE, "%s: store %llu of %llu", what, (unsigned long long)(dst + e), (unsigned long long)len);
                    CHECK(inter.at(dst + e) == ~0ull, "%s: intermediate slot written twice", what);
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
        const uint32_t nbu = 1u << P.lo_bits;
        uint32_t base, cnt;
        const uint32_t lo = bin_base.at(P.shared_entry(b, 0)), hi = bin_base.at(P.shared_entry(b + 1, 0));
        front_bin_range(lo, hi, len, base, cnt);
        CHECK(cnt == hi - lo && (cnt == 0 || base == lo), "%s: bin %u taken as empty", what, b);
        const uint32_t g0 = P.shared_first_bucket(b);
        CHECK((uint64_t)base + cnt <= len, "%s: bin %u ends at %llu", what, b, (unsigned long long)base + cnt);
        for (uint32_t e = 0; e < cnt; ++e) h.at(P.shared_lo(inter.at(base + e)))++;
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
            const uint64_t v = inter.at(base + e);
            CHECK(v != ~0ull, "%s: bin %u reads a slot nothing wrote", what, b);
            const uint32_t pos = cur.at(P.shared_lo(v))++;
            CHECK(pos < cnt, "%s: bin %u position %u of %u", what, b, pos, cnt);
            if (staged) stage.at(pos) = P.shared_final(v);
            else vals_s.at(base + pos) = P.shared_final(v);
        }
        if (staged)
            for (uint32_t e = 0; e < cnt; ++e) vals_s.at(base + e) = stage.at(e);
    }
    // ---- the properties
    std::vector<std::vector<uint32_t>> want(nb);
    uint64_t pairs = 0;
    for (uint64_t i = 0; i < n; ++i)
        msm_signed_digits(sc[i].l, c, w_total, [&](int w, uint32_t d, uint32_t neg) {
            CHECK(d <= half, "%s: digit %u", what, d);
            if (d && w >= w_begin && w < w_begin + wc) {
                want.at(d - 1).push_back((uint32_t)((uint64_t)w * table_n + i) | (neg << 31));
                ++pairs;
            }
        });
    CHECK(bin_base[ntab] == pairs, "%s: %u pairs counted, %llu exist", what, bin_base[ntab], (unsigned long long)pairs);
    uint64_t at = 0;
    for (uint32_t g = 0; g < nb; ++g) {
        CHECK(count[g] == want[g].size(), "%s: bucket %u count %u, direct histogram %zu", what, g, count[g], want[g].size());
        CHECK(start[g] == at, "%s: bucket %u starts at %u, expected %llu", what, g, start[g], (unsigned long long)at);  // key order, no gaps, no overlap
        CHECK((uint64_t)start[g] + count[g] <= len, "%s: bucket %u reaches %llu", what, g, (unsigned long long)start[g] + count[g]);
        CHECK(iota[g] == g && ckey[g] == std::min<uint32_t>(count[g], clamp), "%s: bucket %u iota / key", what, g);
        std::vector<uint32_t> got(vals_s.begin() + start[g], vals_s.begin() + start[g] + count[g]);
        std::sort(got.begin(), got.end());
        std::sort(want[g].begin(), want[g].end());
        CHECK(got == want[g], "%s: bucket %u holds other values than its digits", what, g);
        for (uint32_t v : got) CHECK((uint64_t)(v & 0x7fffffffu) < (uint64_t)w_total * table_n, "%s: value outside the table", what);
        at += count[g];
    }
    return unstaged;
}

int main() {
    const uint64_t sizes[] = {1, 63, 4097, 20011};
    const int cs[] = {11, 16, 19, 20};
    int cases = 0;
    for (int c : cs) {
        const int w_total = (256 + c - 1) / c;
        for (uint64_t n : sizes)
            for (int mix = 0; mix < 8; ++mix) {
                const std::vector<Scalar> sc = make(mix, n, c);
                char what[112];
                snprintf(what, sizeof what, "n %llu c %d %s whole", (unsigned long long)n, c, MIXES[mix]);
                run_case(sc, c, 0, w_total, w_total, n, FRONT_BIN_CAP, what);
                // a prefix of a larger set: the level stride is the set's
                snprintf(what, sizeof what, "n %llu c %d %s prefix of n + 1000", (unsigned long long)n, c, MIXES[mix]);
                run_case(sc, c, 0, w_total, w_total, n + 1000, FRONT_BIN_CAP, what);
                // a range of levels (odd begin, odd count)
                snprintf(what, sizeof what, "n %llu c %d %s levels [3, 8)", (unsigned long long)n, c, MIXES[mix]);
                run_case(sc, c, 3, 5, w_total, n, FRONT_BIN_CAP, what);
                // a bin capacity of one value: every fuller bin takes the unstaged path
                snprintf(what, sizeof what, "n %llu c %d %s tiny capacity", (unsigned long long)n, c, MIXES[mix]);
                const uint64_t unstaged = run_case(sc, c, 0, w_total, w_total, n, 1, what);
                CHECK(n < 63 || mix == 1 || unstaged > 0, "%s: the unstaged path was not taken", what);
                cases += 4;
            }
    }
    // one bucket for a whole vector with the real capacity: a single bin holds every pair of the call, far beyond the staging capacity
    {
        const std::vector<Scalar> sc = make(7, 20011, 20);
        CHECK(run_case(sc, 20, 0, 13, 13, 20011, FRONT_BIN_CAP, "n 20011 c 20 one bucket") > 0, "a 240 000-value bin must exceed the staging capacity");
        ++cases;
    }
    // the plan itself: what must keep the sort, and the default's range
    const uint64_t M = (uint64_t)1 << 20;
    CHECK(!msm_front_plan(1000, 13000, 20, 13, true, true, 1, 1000).on && !msm_front_plan(1000, 13000, 20, 13, false, true, 2, 1000).on, "plan: sort / ineligible");
    CHECK(!msm_front_plan(1000, 26000, 10, 26, true, true, 2, 1000).on && !msm_front_plan(1000, 13000, 21, 13, true, true, 2, 1000).on, "plan: window sizes outside [11, 20]");
    CHECK(!msm_front_plan(1001, 13000, 20, 13, true, true, 2, 1000).on, "plan: more scalars than the table has points");
    CHECK(!msm_front_plan(M, 24 * ((uint64_t)1 << 27), 11, 24, true, true, 2, (uint64_t)1 << 27).on, "plan: index bits");
    CHECK(msm_front_plan(M, 13 * M, 20, 13, true, false, 2, M).on && msm_front_plan(M, 13 * M, 20, 13, true, false, 2, M).shared, "plan: forced");
    CHECK(msm_front_plan(M, 13 * M, 20, 13, true, true, 0, M).on && msm_front_plan(M / 2 + 1, 13 * M, 20, 13, true, true, 0, M).on, "plan: default on");
    CHECK(!msm_front_plan(M, 13 * M, 20, 13, true, false, 0, M).on && !msm_front_plan(M / 2, 13 * M, 20, 13, true, true, 0, M).on &&
              !msm_front_plan(M, 16 * M, 16, 16, true, true, 0, M).on,
          "plan: default off beside other work, below 2^19 points and at other windows");
    CHECK(!msm_front_plan(M, M, 16, 16, true, true, 0).shared && msm_front_plan(M, M, 16, 16, true, true, 0).on, "plan: the plain form is untouched");
    printf("msm_front_shared_check ok: %d cases\n", cases);
    return 0;
}
