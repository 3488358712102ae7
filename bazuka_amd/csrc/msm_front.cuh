// Index arithmetic of the MSM's partition front (msm_impl.cuh section 3d): signed window recoding, the bin of a key, the packed
// intermediate pair, the layout of the per-tile tables and the plan that picks the shapes.  Everything here is plain integer
// arithmetic in __host__ __device__ functions: the kernels of section 3d and the CPU model (tests/host/msm_front_check.hip, built
// with the address and undefined-behaviour sanitizers) run the very same functions, so an index that would leave its array on
// the device leaves it on the CPU first.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BZK_FRONT_HD __host__ __device__
#else
#define BZK_FRONT_HD
#endif

namespace bzk {

// ---- signed c-bit window recoding ---------------------------------------------------------------------------------------------
// digit d in [0, 2^(c-1)] with sign `neg`; raw + carry > 2^(c-1) becomes 2^c - (raw + carry), negative, and carries one into the next window
struct MsmDigit { uint32_t d, neg; };
BZK_FRONT_HD inline MsmDigit msm_recode(uint32_t raw, uint32_t& carry, int c) {
    const uint32_t half = 1u << (c - 1);
    uint32_t d = raw + carry, neg = 0;
    if (d > half) {
        d = (1u << c) - d;
        neg = 1;
        carry = 1;
    } else {
        carry = 0;
    }
    return MsmDigit{d, neg};
}
// the w_total signed digits of a canonical 256-bit scalar (8 x 32-bit limbs, little-endian), lowest window first: emit(w, d, neg).
// The carry out of the top window is dropped (the callers bring the scalar under r < 2^255 first).
template <class F>
BZK_FRONT_HD inline void msm_signed_digits(const uint32_t* l, int c, int w_total, F&& emit) {
    const uint32_t mask = (1u << c) - 1;
    uint64_t buf = 0;
    int cnt = 0, w = 0;
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        buf |= (uint64_t)l[j] << cnt;
        cnt += 32;
        while (cnt >= c && w < w_total) {
            const MsmDigit g = msm_recode((uint32_t)buf & mask, carry, c);
            emit(w, g.d, g.neg);
            ++w;
            buf >>= c;
            cnt -= c;
        }
    }
    while (w < w_total) {
        const MsmDigit g = msm_recode((uint32_t)buf & mask, carry, c);
        emit(w, g.d, g.neg);
        ++w;
        buf >>= c;
    }
}

// ---- shapes ---------------------------------------------------------------------------------------------------------------------
static constexpr uint32_t FRONT_TILE = 4096;       // scalars per workgroup of the histogram and scatter passes
static constexpr uint32_t FRONT_THREADS = 1024;    // lanes of those workgroups (FRONT_TILE / FRONT_THREADS scalars per lane)
static constexpr uint32_t FRONT_GW = 4;            // windows the scatter pass stages in LDS at a time (FRONT_TILE * FRONT_GW values)
static constexpr uint32_t FRONT_HI_MAX = 7;        // bins per window <= 128: a (tile, window, bin) run is >= 32 values = 128 bytes on average
static constexpr uint32_t FRONT_LO_MAX = 10;       // buckets per bin <= 1024 (the bin pass's LDS histogram)
static constexpr uint32_t FRONT_BIN_THREADS = 512; // lanes of a bin-pass workgroup
static constexpr uint32_t FRONT_BIN_CAP = 12288;   // values a bin-pass workgroup can stage in LDS (48 KiB); fuller bins are scattered straight to memory
static constexpr uint32_t FRONT_SCAN_BINS = 16;    // bins per workgroup of the scan pass (16 lanes x 4 bytes = one 64-byte line per tile row)
static constexpr uint32_t FRONT_SCAN_PARTS = 16;   // tile ranges per bin in that workgroup
// a call whose windows share ONE bucket set (a full window table: FrontPlan::shared)
static constexpr uint32_t FRONT_GW_SHARED = 4;        // windows its scatter pass stages at a time (FRONT_TILE * FRONT_GW_SHARED tile-local 32-bit words: the same 64 KiB)
static constexpr uint32_t FRONT_SHARED_HI_MAX = 9;    // bins <= 512 (c = 20: 2^19 keys = 512 bins of 1024 buckets)
static constexpr uint32_t FRONT_SHARED_TAB_MAX = 4096; // entries of a tile's row of the tables: bins x window groups (c = 20: 512 x 4 = 2048)
static constexpr uint32_t FRONT_TABLE_LEVEL_BITS = 5;  // the level of a pair inside its call, above lo in the staged word and in the 64-bit pair
static constexpr uint32_t FRONT_TABLE_LEVELS_MAX = 24; // levels of one call (c = 11: 24 windows)
static constexpr uint32_t FRONT_TABLE_CELLS_MAX = 18432;  // (bucket, level) counters of a bin-pass workgroup, 72 KiB: c = 15 has 1024 buckets x 18 levels, c = 20 1024 x 13
static constexpr uint32_t FRONT_TABLE_BIN_THREADS = 1024; // lanes of a bin-pass workgroup of a table call
static constexpr uint32_t FRONT_TABLE_LDS_WORDS = 40944;  // that workgroup's cells and, behind them, its stage of 32-bit values: the CU's 160 KiB less the scan's 16 words
static constexpr uint32_t FRONT_TABLE_BIN_HELD = 27;      // pairs a lane keeps in registers while its bin is ordered in the stage (27 x 1024 >= 40944 - 13312: c = 20)
static constexpr uint32_t FRONT_TABLE_BIN_UNROLL = 4;     // strides whose loads are in flight together in the sweeps of a bin too full for the stage

// Key k = d - 1 in [0, 2^(c-1)) = hi : lo.  A bin is a (window of the group, hi) pair, bins are window-major; the buckets of a bin are its 2^lo_bits keys.
// Intermediate pair (32 bits, no key array): base index in idx_bits, lo above it, the sign in bit 31 - the window is the bin's.
struct FrontPlan {
    bool on = false;  // false: this call keeps the radix sort
    uint32_t hi_bits = 0, lo_bits = 0, idx_bits = 0;
    uint32_t n_tiles = 0;
    BZK_FRONT_HD uint32_t bins_per_window() const { return 1u << hi_bits; }
    BZK_FRONT_HD uint32_t nbins(uint32_t windows) const { return windows << hi_bits; }
    BZK_FRONT_HD uint32_t bin_of(uint32_t lw, uint32_t key) const { return (lw << hi_bits) | (key >> lo_bits); }
    BZK_FRONT_HD uint32_t lo_of(uint32_t key) const { return key & ((1u << lo_bits) - 1); }
    BZK_FRONT_HD uint32_t pack(uint32_t index, uint32_t key, uint32_t neg) const { return index | (lo_of(key) << idx_bits) | (neg << 31); }
    BZK_FRONT_HD uint32_t packed_lo(uint32_t v) const { return (v >> idx_bits) & ((1u << lo_bits) - 1); }
    // the final value of the accumulation's gather list: index | window of the group << 27 | sign << 31 (clean under the mask 0x07ffffff)
    BZK_FRONT_HD uint32_t final_value(uint32_t v, uint32_t lw) const { return (v & ((1u << idx_bits) - 1)) | (lw << 27) | (v & 0x80000000u); }
    // first bucket (window-major bucket index of the call: lw * half + key) of bin b
    BZK_FRONT_HD uint32_t first_bucket(uint32_t b, uint32_t half) const { return (b >> hi_bits) * half + ((b & ((1u << hi_bits) - 1)) << lo_bits); }
    BZK_FRONT_HD size_t table_at(uint32_t tile, uint32_t bin, uint32_t nbins_) const { return (size_t)tile * nbins_ + bin; }

    // ---- shared bucket set: every window of the call feeds the SAME 2^(c-1) buckets from its own level of a window table (msm_run with a full table).
    // A bin is the key's high bits alone.  The scatter pass stages FRONT_GW_SHARED windows at a time, so a tile leaves `groups` runs per bin: the tables hold
    // one entry per (bin, window group), bin-major - the groups of a bin are adjacent, and the scan over the entries lays every bin out contiguously.
    // Intermediate pair (64 bits): the final gather word - table index w * table_n + i, sign in bit 31 - in the low half, lo above it, and above lo the level
    // inside the call (table_widen below: what the kernels write; shared_pack is the same pair without the level).
    bool shared = false;
    uint32_t table_n = 0;  // points per level of the table (the set's n, not the call's)
    uint32_t groups = 0;   // window groups of the call: ceil(windows / FRONT_GW_SHARED)
    BZK_FRONT_HD uint32_t shared_bins() const { return 1u << hi_bits; }
    BZK_FRONT_HD uint32_t shared_tab() const { return groups << hi_bits; }
    BZK_FRONT_HD uint32_t shared_group(uint32_t w) const { return w / FRONT_GW_SHARED; }
    BZK_FRONT_HD uint32_t shared_bin(uint32_t key) const { return key >> lo_bits; }
    BZK_FRONT_HD uint32_t shared_entry(uint32_t bin, uint32_t group) const { return bin * groups + group; }
    BZK_FRONT_HD uint64_t shared_pack(uint32_t w, uint32_t i, uint32_t key, uint32_t neg) const {
        return (uint64_t)(w * table_n + i) | ((uint64_t)neg << 31) | ((uint64_t)lo_of(key) << 32);
    }
    BZK_FRONT_HD uint32_t shared_lo(uint64_t v) const { return (uint32_t)(v >> 32) & ((1u << lo_bits) - 1); }
    // the final value of the accumulation's gather list: index | sign << 31 (clean under the mask 0x7fffffff)
    BZK_FRONT_HD uint32_t shared_final(uint64_t v) const { return (uint32_t)v; }
    BZK_FRONT_HD uint32_t shared_first_bucket(uint32_t b) const { return b << lo_bits; }

    // ---- what the kernels of a table call stage and rank by: the pair carries its level of the call (lw = w - w_begin < levels), so that the bin pass
    // ranks over (bucket, level) cells and leaves every bucket level-major - the pair sort's order - whatever order the pairs arrive in.
    uint32_t levels = 0;  // levels of one pass of the call: the stride of a bucket's cells
    // the scatter pass's staged word (32 bits, tile-local): index inside the tile in 12 bits, lw, the sign, lo - 28 bits at most
    BZK_FRONT_HD uint32_t table_stage(uint32_t t, uint32_t lw, uint32_t key, uint32_t neg) const {
        return t | (lw << 12) | (neg << (12 + FRONT_TABLE_LEVEL_BITS)) | (lo_of(key) << (13 + FRONT_TABLE_LEVEL_BITS));
    }
    // widened on the way out to the 64-bit pair: shared_pack's fields (shared_lo / shared_final read it unchanged) with lw above lo, in bits 42 .. 46
    BZK_FRONT_HD uint64_t table_widen(uint32_t s, uint32_t tile, uint32_t w_begin) const {
        const uint32_t t = s & (FRONT_TILE - 1), lw = (s >> 12) & ((1u << FRONT_TABLE_LEVEL_BITS) - 1), neg = (s >> (12 + FRONT_TABLE_LEVEL_BITS)) & 1u;
        const uint32_t lo = s >> (13 + FRONT_TABLE_LEVEL_BITS);
        return (uint64_t)((w_begin + lw) * table_n + tile * FRONT_TILE + t) | ((uint64_t)neg << 31) | ((uint64_t)lo << 32) | ((uint64_t)lw << (32 + FRONT_LO_MAX));
    }
    BZK_FRONT_HD uint32_t table_level(uint64_t v) const { return (uint32_t)(v >> (32 + FRONT_LO_MAX)) & ((1u << FRONT_TABLE_LEVEL_BITS) - 1); }
    // cells of a bin, bucket-major and level-minor: the exclusive scan over them gives every bucket's start and every cell's rank base
    BZK_FRONT_HD uint32_t table_cells() const { return levels << lo_bits; }
    BZK_FRONT_HD uint32_t table_cell(uint64_t v) const { return shared_lo(v) * levels + table_level(v); }
};
static_assert(FRONT_TILE == 4096 && 13 + FRONT_TABLE_LEVEL_BITS + FRONT_LO_MAX <= 32, "the staged word of a table call: 12 index bits, level, sign, lo");
static_assert(FRONT_TABLE_LEVELS_MAX <= (1u << FRONT_TABLE_LEVEL_BITS), "a level fits its field");
static_assert(FRONT_TABLE_CELLS_MAX < FRONT_TABLE_LDS_WORDS && 4 * (FRONT_TABLE_LDS_WORDS + FRONT_TABLE_BIN_THREADS / 64) <= 160 * 1024, "the bin pass's LDS");

// tiles [t0, t1) of part q (of FRONT_SCAN_PARTS) in the scan pass
BZK_FRONT_HD inline void front_scan_range(uint32_t n_tiles, uint32_t q, uint32_t& t0, uint32_t& t1) {
    const uint32_t per = (n_tiles + FRONT_SCAN_PARTS - 1) / FRONT_SCAN_PARTS;
    t0 = q * per < n_tiles ? q * per : n_tiles;
    t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
}

// ---- the bin pass ---------------------------------------------------------------------------------------------------------------
// bin b holds [lo, hi) = [bin_base[b], bin_base[b + 1]) of the len intermediate pairs.  A range that would leave the array cannot happen (the tables count
// what the scatter pass wrote); were it to, the bin is taken as empty, so that its buckets still get a start, a zero count, their iota and population key.
BZK_FRONT_HD inline void front_bin_range(uint32_t lo, uint32_t hi, uint64_t len, uint32_t& base, uint32_t& cnt) {
    const bool ok = lo <= hi && (uint64_t)hi <= len;
    base = ok ? lo : 0u;
    cnt = ok ? hi - lo : 0u;
}
// a bin of cnt values is ordered in LDS while it fits `cap` values (the kernel: FRONT_BIN_CAP), and stored through the running cursors otherwise
BZK_FRONT_HD inline bool front_bin_staged(uint32_t cnt, uint32_t cap) { return cnt <= (cap < FRONT_BIN_CAP ? cap : FRONT_BIN_CAP); }
// a table call's bin of ncell (bucket, level) cells is ordered in LDS while its values fit behind the cells and in the lanes' registers, and stored through
// the running cursors otherwise
BZK_FRONT_HD inline uint32_t front_table_bin_cap(uint32_t ncell) {
    const uint32_t room = ncell < FRONT_TABLE_LDS_WORDS ? FRONT_TABLE_LDS_WORDS - ncell : 0u, held = FRONT_TABLE_BIN_HELD * FRONT_TABLE_BIN_THREADS;
    return room < held ? room : held;
}
// the population key of a bucket of cn values (what msm_count_kernel writes on the sort path)
BZK_FRONT_HD inline uint32_t front_pop_key(uint32_t cn, uint32_t clamp) { return cn < clamp ? cn : clamp; }

// The one place that decides whether a call's pairs are bucketed by the partition passes, and in which shapes.
//   n_index   exclusive bound of the base indices the values carry (points, plus group sums where a call has them)
//   eligible  the call takes the plain window-in-value digits path: no table, no endomorphism form, no de-duplication
//   alone     no BZK_F_THROUGHPUT hint and not a window range of a split call (independent calls on other contexts are not seen here: measured below)
//   mode      bzk_ctx::msm_front: 0 = by the measured crossover below, 1 = always the sort, 2 = the partition wherever it can run
// hi = min(7, c - 5), lo = c - 1 - hi: c = 16 gives 128 bins of 256 buckets per window; 9 <= c <= 17 keeps lo <= FRONT_LO_MAX and >= 16 bins per window
// (the scan pass takes FRONT_SCAN_BINS bins per workgroup).  The packed intermediate must hold the index beside lo: n_index <= 2^(31 - lo).
//   table_n   0 for a plain call; the level stride of the full window table for a call whose `windows` levels share one bucket set (eligible then means:
//             a full table, no de-duplication).  Such a call: 11 <= c <= 20, lo = min(10, c - 5), hi = c - 1 - lo in [4, 9], every window in one pass,
//             at most FRONT_TABLE_LEVELS_MAX of them, and levels << lo (bucket, level) cells in the bin pass's LDS: at most FRONT_TABLE_CELLS_MAX
inline FrontPlan msm_front_plan(uint64_t n, uint64_t n_index, int c, int windows, bool eligible, bool alone, int mode, uint64_t table_n = 0) {
    FrontPlan P;
    if (table_n) {
        if (!eligible || mode == 1 || c < 11 || c > 20 || windows < 1 || (uint32_t)windows > FRONT_TABLE_LEVELS_MAX || n == 0 || n > table_n ||
            n > ((uint64_t)1 << 24) || (uint64_t)windows * table_n >= ((uint64_t)1 << 31) || n_index > ((uint64_t)1 << 31))
            return P;
        P.lo_bits = (uint32_t)(c - 5) < FRONT_LO_MAX ? (uint32_t)(c - 5) : FRONT_LO_MAX;
        P.hi_bits = (uint32_t)(c - 1) - P.lo_bits;
        P.idx_bits = 31;
        P.table_n = (uint32_t)table_n;
        P.groups = ((uint32_t)windows + FRONT_GW_SHARED - 1) / FRONT_GW_SHARED;
        P.levels = (uint32_t)windows;
        // the bin pass keeps one LDS counter per (bucket, level) cell: a shape whose cells do not fit keeps the sort (none of c = 11 .. 20 does: c = 15 has
        // the most, 1024 x 18 = FRONT_TABLE_CELLS_MAX)
        if (P.hi_bits > FRONT_SHARED_HI_MAX || P.shared_tab() > FRONT_SHARED_TAB_MAX || P.table_cells() > FRONT_TABLE_CELLS_MAX) return P;
        P.n_tiles = (uint32_t)((n + FRONT_TILE - 1) / FRONT_TILE);
        P.shared = true;
        // Measured (profiles/msm_table_front_ab.json: 2^20 points, c = 20, one resident set with its table, one process, three alternations, medians of
        // 25 calls): sort 3.146 - 3.153 ms, partition 2.870 - 2.889 ms (with 2 levels per scatter round and a bin pass ranking by bucket alone, a barrier per
        // stride: 3.171 - 3.241 against 3.040 - 3.125).  The chain before the accumulation: sort 0.49 ms, partition 0.23 (histogram 0.028 + scan 0.012 +
        // scatter 0.097 + bins 0.096; before: 0.029 + 0.012 + 0.135 + 0.217); msm_accumulate 1.94 - 1.95 ms in the sort's order, 1.95 - 1.96 in this one's
        // (level-major too), 1.98 - 1.99 in the old group-major one.  Kernels: scatter 128 VGPRs, 90 176 B LDS, one spilled register; bin pass 82 VGPRs,
        // 163 840 B LDS, no scratch.  Not measured: other window sizes for speed, the bin pass with a barrier per stride.
        // So by default: the table calls of that shape that run alone; everything else keeps the sort
        P.on = mode == 2 || (alone && c == 20 && n > ((uint64_t)1 << 19) && n <= ((uint64_t)1 << 20));
        return P;
    }
    if (!eligible || mode == 1 || c < 9 || c > 17 || windows < 1 || windows > 16 || n == 0 || n > ((uint64_t)1 << 24)) return P;
    P.hi_bits = (uint32_t)(c - 5) < FRONT_HI_MAX ? (uint32_t)(c - 5) : FRONT_HI_MAX;
    P.lo_bits = (uint32_t)(c - 1) - P.hi_bits;
    P.idx_bits = 31 - P.lo_bits < 27 ? 31 - P.lo_bits : 27;  // the final value keeps 27 index bits under the window
    if (n_index > ((uint64_t)1 << P.idx_bits)) return P;
    P.n_tiles = (uint32_t)((n + FRONT_TILE - 1) / FRONT_TILE);
    if (mode == 2) {
        P.on = true;
        return P;
    }
    // Measured crossover (uniform scalars; profiles/msm_front_partition_ab.json), ms per call sort -> partition:
    //   resident G1 set, same process, alternating: 2^20 points (c = 16)  3.41 -> 3.26     2^21  6.43 -> 6.22     2^22  12.18 -> 11.90 (bins beyond
    //     FRONT_BIN_CAP: the unstaged bin pass, still ahead);
    //   2^20 over raw bases (the conversion runs on the side stream beside the passes) 3.38 - 3.48 -> 3.25 - 3.33; G2 2^20 10.38 - 10.46 -> 10.11 - 10.38;
    //     two independent 2^20 calls in flight on two contexts 3.27 - 3.32 -> 3.10 - 3.18 per call, four 3.09 - 3.11 -> 2.90 - 3.00: all of these count as alone;
    //   2^18 (c = 14) 1.74 - 1.77 -> 1.94 - 2.01 and 2^19 (c = 15) 2.35 - 2.40 -> 2.68 - 2.78 (medians of three runs each, the shipped kernels): those calls
    //     run as two window ranges in flight: the sort stays.  The likely reason - beside the other range's accumulation the passes' large workgroups
    //     (80 KiB / 56 KiB of LDS) wait for a CU where rocPRIM's small ones slip in - is a hypothesis: no trace of those calls was taken;
    //   2^24: the index does not fit beside lo (n_index > 2^23): the sort stays.
    // So: c = 16 calls of 2^20 .. 2^22 points that are no window range of a split call and carry no throughput hint.  Smaller window sizes and the prover's
    // overlapping calls keep the sort.
    P.on = alone && c >= 16 && n >= ((uint64_t)1 << 20) && n <= ((uint64_t)1 << 22);
    return P;
}

}  // namespace bzk
