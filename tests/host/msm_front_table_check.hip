// CPU model of the passes a table call's partition front runs (bazuka_amd/csrc/msm_impl.cuh section 3d, FrontPlan::shared): the histogram and scan over
// (bin, group of FRONT_GW_SHARED levels) entries, the scatter pass that stages tile-local 32-bit words and widens them to 64-bit pairs carrying their level, and
// the bin pass that ranks by (bucket, level) cells without a barrier - as plain loops over the very __host__ __device__ index functions the kernels use
// (msm_front.cuh), every array sized exactly as the kernel's __shared__ array or the call's workspace.  Built with -fsanitize=address,undefined and run as a
// program of its own (tests/test_msm_front_table_cpu.py): an index that would leave its array on the device aborts here.  The lanes of the bin pass's second
// sweep are walked BACKWARDS: nothing the pass promises may depend on the order in which the lanes arrive.  Checked per case: every non-zero digit of every
// requested level lands exactly once inside its own bucket's [start, start + count) as table index | sign, start is gap-free in key order, count equals a
// direct histogram, iota / population keys are what msm_count wrote, the levels inside every bucket are non-decreasing, no cell or stage index leaves its
// array, and a shape the plan refuses is refused.
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
// the eight mixes of msm_front_shared_check.hip
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

struct Ran { uint32_t fullest, staged, direct; };  // the fullest cell of the call; non-empty bins ordered in the stage resp. stored through the cursors
// levels [w_begin, w_begin + wc) of a table of w_total levels x table_n points, the first sc.size() points of it
static Ran run_case(const std::vector<Scalar>& sc, int c, int w_begin, int wc, int w_total, uint64_t table_n, const char* what) {
    const uint64_t n = sc.size();
    const FrontPlan P = msm_front_plan(n, (uint64_t)w_total * table_n, c, wc, true, true, 2, table_n);
    CHECK(P.on && P.shared, "%s: plan refuses n %llu c %d", what, (unsigned long long)n, c);
    const uint32_t half = 1u << (c - 1), nbins = P.shared_bins(), ntab = P.shared_tab(), nb = half, ncell = P.table_cells();
    const uint64_t len = (uint64_t)wc * n;
    CHECK(ntab % FRONT_SCAN_BINS == 0 && ntab <= FRONT_SHARED_TAB_MAX && nbins <= (1u << FRONT_SHARED_HI_MAX) && P.lo_bits <= FRONT_LO_MAX &&
              P.hi_bits + P.lo_bits == (uint32_t)c - 1 && P.groups * FRONT_GW_SHARED >= (uint32_t)wc && P.levels == (uint32_t)wc &&
              ncell <= FRONT_TABLE_CELLS_MAX && (uint32_t)wc <= FRONT_TABLE_LEVELS_MAX,
          "%s: shapes", what);
    // the workspace of the call, as msm_run declares it
    std::vector<uint32_t> tile_hist((size_t)P.n_tiles * ntab, 0xdeadbeefu), tile_off((size_t)P.n_tiles * ntab, 0xdeadbeefu), bin_total(ntab, 0xdeadbeefu),
        bin_base(ntab + 1, 0xdeadbeefu), vals_s(len, 0xffffffffu), start(nb, 0xdeadbeefu), count(nb, 0xdeadbeefu), iota(nb, 0xdeadbeefu), ckey(nb, 0xdeadbeefu);
    std::vector<uint64_t> inter(len, ~0ull);
    // 1. histogram (msm_front_hist_kernel<true>)
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
    // 2. scan (msm_front_scan_kernel, over the entries)
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
    // 3. scatter (msm_front_scatter_kernel<true>): 32-bit tile-local words in the stage, widened as a run is stored
    constexpr uint32_t STAGE = FRONT_TILE * FRONT_GW_SHARED, GB = 1u << FRONT_SHARED_HI_MAX;
    for (uint32_t tile = 0; tile < P.n_tiles; ++tile) {
        std::vector<uint32_t> stage(STAGE, 0xffffffffu);
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
                            const uint32_t word = P.table_stage(j * FRONT_THREADS + tid, (uint32_t)(w - w_begin), d - 1, neg);
                            CHECK(word < (1u << 28), "%s: staged word %08x wider than 28 bits", what, word);
                            stage.at(pos) = word;
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
                    inter.at(dst + e) = P.table_widen(stage.at(src + e), tile, (uint32_t)w_begin);
                }
            }
        }
    }
    // 4. bin pass (msm_front_table_bins_kernel): lanes and strides as the kernel walks them - a bin that fits the stage is held in the lanes' registers and
    //    ordered in LDS, a fuller one takes two sweeps and stores through the cursors -, the ranking sweep backwards
    constexpr uint32_t T = FRONT_TABLE_BIN_THREADS, U = FRONT_TABLE_BIN_UNROLL, H = FRONT_TABLE_BIN_HELD;
    const uint32_t clamp = len / nb <= 64 ? 255u : 65535u, cap = front_table_bin_cap(ncell);
    CHECK((uint64_t)ncell + cap <= FRONT_TABLE_LDS_WORDS && cap <= H * T, "%s: a stage of %u values behind %u cells", what, cap, ncell);
    Ran ran = {};
    std::vector<uint32_t> lds(FRONT_TABLE_LDS_WORDS, 0xdeadbeefu);  // the workgroup's LDS: the cells, the stage behind them
    std::vector<uint64_t> held((size_t)T * H);                       // the lanes' registers
    for (uint32_t b = 0; b < nbins; ++b) {
        const uint32_t nbu = 1u << P.lo_bits;
        uint32_t base, cnt;
        const uint32_t lo = bin_base.at(P.shared_entry(b, 0)), hi = bin_base.at(P.shared_entry(b + 1, 0));
        front_bin_range(lo, hi, len, base, cnt);
        CHECK(cnt == hi - lo && (cnt == 0 || base == lo), "%s: bin %u taken as empty", what, b);
        const uint32_t g0 = P.shared_first_bucket(b);
        CHECK((uint64_t)base + cnt <= len, "%s: bin %u ends at %llu", what, b, (unsigned long long)base + cnt);
        const bool staged = cnt <= cap;
        if (cnt) ++(staged ? ran.staged : ran.direct);
        for (uint32_t k = 0; k < ncell; ++k) lds.at(k) = 0;
        uint32_t seen = 0;
        auto count_one = [&](uint64_t v) {
            CHECK(v != ~0ull, "%s: bin %u reads a slot nothing wrote", what, b);
            const uint32_t cl = P.table_cell(v);
            CHECK(cl < ncell, "%s: bin %u cell %u of %u", what, b, cl, ncell);
            ran.fullest = std::max(ran.fullest, ++lds.at(cl));
            ++seen;
        };
        if (staged) {
            for (uint32_t tid = 0; tid < T; ++tid)
                for (uint32_t u = 0; u < H; ++u) held.at((size_t)tid * H + u) = tid + u * T < cnt ? inter.at(base + tid + u * T) : ~0ull;
            for (uint32_t tid = 0; tid < T; ++tid)
                for (uint32_t u = 0; u < H; ++u)
                    if (tid + u * T < cnt) count_one(held.at((size_t)tid * H + u));
        } else {
            for (uint32_t tid = 0; tid < T; ++tid)
                for (uint32_t e0 = tid; e0 < cnt; e0 += T * U)
                    for (uint32_t u = 0; u < U; ++u)
                        if (e0 + u * T < cnt) count_one(inter.at(base + e0 + u * T));
        }
        CHECK(seen == cnt, "%s: bin %u: the counting sweep visits %u of %u", what, b, seen, cnt);
        excl_scan(lds.data(), lds.data(), ncell, nullptr);
        for (uint32_t k = 0; k < nbu; ++k) {
            const uint32_t g = g0 + k, at = lds.at(k * P.levels), cn = (k + 1 < nbu ? lds.at((k + 1) * P.levels) : cnt) - at;
            CHECK(g < nb, "%s: bucket %u of %u", what, g, nb);
            CHECK(start.at(g) == 0xdeadbeefu, "%s: bucket %u written twice", what, g);
            start.at(g) = base + at;
            count.at(g) = cn;
            iota.at(g) = g;
            ckey.at(g) = front_pop_key(cn, clamp);
        }
        auto rank_one = [&](uint64_t v) {
            const uint32_t cl = P.table_cell(v);
            CHECK(cl < ncell, "%s: bin %u cell %u of %u", what, b, cl, ncell);
            const uint32_t pos = lds.at(cl)++;
            CHECK(pos < cnt, "%s: bin %u position %u of %u", what, b, pos, cnt);
            if (staged) {
                CHECK(pos < cap, "%s: bin %u position %u beyond the stage of %u", what, b, pos, cap);
                lds.at(ncell + pos) = P.shared_final(v);
            } else {
                CHECK(vals_s.at(base + pos) == 0xffffffffu, "%s: bin %u position %u written twice", what, b, pos);
                vals_s.at(base + pos) = P.shared_final(v);
            }
        };
        if (staged) {
            for (uint32_t tid = T; tid-- > 0;)
                for (uint32_t u = H; u-- > 0;)
                    if (tid + u * T < cnt) rank_one(held.at((size_t)tid * H + u));
            for (uint32_t e = 0; e < cnt; ++e) vals_s.at(base + e) = lds.at(ncell + e);
        } else {
            for (uint32_t tid = T; tid-- > 0;)
                for (uint32_t e0 = tid; e0 < cnt; e0 += T * U)
                    for (uint32_t u = U; u-- > 0;)
                        if (e0 + u * T < cnt) rank_one(inter.at(base + e0 + u * T));
        }
    }
    // ---- the properties
    std::vector<uint64_t> want, got;  // (bucket, value) of every pair
    for (uint64_t i = 0; i < n; ++i)
        msm_signed_digits(sc[i].l, c, w_total, [&](int w, uint32_t d, uint32_t neg) {
            CHECK(d <= half, "%s: digit %u", what, d);
            if (d && w >= w_begin && w < w_begin + wc) want.push_back((uint64_t)(d - 1) << 32 | (uint32_t)((uint64_t)w * table_n + i) | (neg << 31));
        });
    CHECK(bin_base[ntab] == want.size(), "%s: %u pairs counted, %zu exist", what, bin_base[ntab], want.size());
    std::vector<uint32_t> direct(nb, 0);
    for (uint64_t p : want) direct.at(p >> 32)++;
    uint64_t at = 0;
    for (uint32_t g = 0; g < nb; ++g) {
        CHECK(count[g] == direct[g], "%s: bucket %u count %u, direct histogram %u", what, g, count[g], direct[g]);
        CHECK(start[g] == at, "%s: bucket %u starts at %u, expected %llu", what, g, start[g], (unsigned long long)at);  // key order, no gaps, no overlap
        CHECK((uint64_t)start[g] + count[g] <= len, "%s: bucket %u reaches %llu", what, g, (unsigned long long)start[g] + count[g]);
        CHECK(iota[g] == g && ckey[g] == std::min<uint32_t>(count[g], clamp), "%s: bucket %u iota / key", what, g);
        uint64_t level = 0;
        for (uint32_t e = 0; e < count[g]; ++e) {
            const uint32_t v = vals_s.at(start[g] + e);
            const uint64_t index = v & 0x7fffffffu;
            CHECK(index < (uint64_t)w_total * table_n, "%s: value outside the table", what);
            CHECK(index / table_n >= level, "%s: bucket %u: level %llu behind level %llu", what, g, (unsigned long long)(index / table_n), (unsigned long long)level);
            level = index / table_n;
            got.push_back((uint64_t)g << 32 | v);
        }
        at += count[g];
    }
    std::sort(want.begin(), want.end());
    std::sort(got.begin(), got.end());
    CHECK(got == want, "%s: the buckets hold other values than their digits", what);
    return ran;
}

int main() {
    const uint64_t sizes[] = {1, 63, 4097, 20011};
    int cases = 0;
    for (int c = 11; c <= 20; ++c) {  // every window size: the cells of a bin are levels x 2^lo
        const int w_total = (256 + c - 1) / c;
        for (uint64_t n : sizes)
            for (int mix = 0; mix < 8; ++mix) {
                const std::vector<Scalar> sc = make(mix, n, c);
                char what[112];
                snprintf(what, sizeof what, "n %llu c %d %s whole", (unsigned long long)n, c, MIXES[mix]);
                run_case(sc, c, 0, w_total, w_total, n, what);
                // a prefix of a larger set: the level stride is the set's
                snprintf(what, sizeof what, "n %llu c %d %s prefix of n + 1000", (unsigned long long)n, c, MIXES[mix]);
                run_case(sc, c, 0, w_total, w_total, n + 1000, what);
                // a range of levels (odd begin, odd count): the level a pair carries is the one inside the call
                snprintf(what, sizeof what, "n %llu c %d %s levels [3, 8)", (unsigned long long)n, c, MIXES[mix]);
                run_case(sc, c, 3, 5, w_total, n, what);
                cases += 3;
            }
    }
    // a bin of exactly the stage's capacity, one value fewer and one more, at every c: k scalars with the digit in every window, one with it in the lowest r
    for (int c = 11; c <= 20; ++c) {
        const int w_total = (256 + c - 1) / c, per = 254 / c;
        const uint32_t cap = front_table_bin_cap(msm_front_plan(1, w_total, c, w_total, true, true, 2, 1).table_cells());
        for (uint32_t cnt : {cap - 1, cap, cap + 1}) {
            std::vector<Scalar> sc(cnt / per, repeated_digit(c, 5));
            Scalar last = {};
            for (uint32_t w = 0; w < cnt % per; ++w)
                for (int bit = 0; bit < c; ++bit)
                    if ((5u >> bit) & 1) last.l[(w * c + bit) / 32] |= 1u << ((w * c + bit) % 32);
            sc.push_back(last);
            char what[112];
            snprintf(what, sizeof what, "c %d: one bin of %u values, stage of %u", c, cnt, cap);
            const Ran r = run_case(sc, c, 0, w_total, w_total, sc.size(), what);
            CHECK(r.staged + r.direct == 1 && r.staged == (cnt <= cap ? 1u : 0u), "%s: staged %u, direct %u", what, r.staged, r.direct);
            ++cases;
        }
    }
    // one bucket for a whole vector: a single bin holds every pair of the call, one cell per level holds n of them
    {
        const std::vector<Scalar> sc = make(7, 20011, 20);
        const Ran r = run_case(sc, 20, 0, 13, 13, 20011, "n 20011 c 20 one bucket");
        CHECK(r.fullest == 20011 && r.direct == 1 && r.staged == 0, "a level of the one-bucket vector fills one cell with every scalar, its bin exceeds the stage");
        ++cases;
    }
    // the plan: every c in [11, 20] runs the passes with its own level count, and what does not fit the bin pass's cells or the level field keeps the sort
    const uint64_t M = (uint64_t)1 << 20;
    for (int c = 11; c <= 20; ++c) {
        const int w = (256 + c - 1) / c;
        const FrontPlan P = msm_front_plan(M, (uint64_t)w * M, c, w, true, true, 2, M);
        CHECK(P.on && P.shared && P.levels == (uint32_t)w && P.table_cells() <= FRONT_TABLE_CELLS_MAX, "plan: c %d", c);
    }
    CHECK(msm_front_plan(M, 18 * M, 15, 18, true, true, 2, M).table_cells() == FRONT_TABLE_CELLS_MAX, "plan: c = 15 fills the cells");
    CHECK(!msm_front_plan(1000, 19000, 15, 19, true, true, 2, 1000).on && !msm_front_plan(1000, 24000, 16, 24, true, true, 2, 1000).on,
          "plan: more cells than the bin pass holds");
    CHECK(!msm_front_plan(1000, 25000, 11, 25, true, true, 2, 1000).on, "plan: more levels than the level field holds");
    CHECK(!msm_front_plan(1000, 26000, 10, 26, true, true, 2, 1000).on && !msm_front_plan(1000, 13000, 21, 13, true, true, 2, 1000).on, "plan: window sizes outside [11, 20]");
    CHECK(!msm_front_plan(1000, 13000, 20, 13, true, true, 1, 1000).on, "plan: the sort when asked for");
    CHECK(!msm_front_plan(M, ((uint64_t)1 << 31) + 1, 20, 13, true, true, 2, M).on, "plan: a table index beyond 31 bits");
    CHECK(msm_front_plan(M, 13 * M, 20, 13, true, true, 0, M).on && !msm_front_plan(M, 13 * M, 20, 13, true, false, 0, M).on, "plan: the default");
    printf("msm_front_table_check ok: %d cases\n", cases);
    return 0;
}
