// Staging rounds of a batched call: which records go up together.  Index arithmetic only, plain C++ (checked stand-alone by
// tests/host/rounds_check.hip); the loop over the rounds is bzk_stage.h's, everything a round launches stays with the callers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace bzk {

// The starts of the rounds of n records, greedily: a round always takes its first record, then the next one while it holds fewer than
// max_records and its summed weight stays at most max_weight.  chunk_at begins with 0 and ends with n ({0} for n == 0); round c is
// [chunk_at[c], chunk_at[c + 1]).  weight(i) is what record i counts towards max_weight.
template <class W>
std::vector<uint64_t> cut_rounds(uint64_t n, uint64_t max_records, uint64_t max_weight, W weight) {
    std::vector<uint64_t> chunk_at(1, 0);
    for (uint64_t a = 0; a < n;) {
        uint64_t b = a + 1, sum = weight(a);
        for (; b < n && b - a < max_records; ++b) {
            const uint64_t w = weight(b);
            if (sum > max_weight || w > max_weight - sum) break;  // sum + w <= max_weight, written so that it cannot wrap
            sum += w;
        }
        chunk_at.push_back(b);
        a = b;
    }
    return chunk_at;
}

// the usual weight: record i's own bytes, from n + 1 byte offsets
inline auto lengths(const uint64_t* off) {
    return [off](uint64_t i) { return off[i + 1] - off[i]; };
}

// what the longest round needs: cap records, and cap_bytes = the largest off[b] - off[a] over the rounds [a, b) (off: n + 1 byte offsets; null: 0)
struct RoundCaps {
    uint64_t cap = 0, cap_bytes = 0;
};
inline RoundCaps round_caps(const std::vector<uint64_t>& chunk_at, const uint64_t* off) {
    RoundCaps r;
    for (size_t c = 0; c + 1 < chunk_at.size(); ++c) {
        const uint64_t a = chunk_at[c], b = chunk_at[c + 1];
        r.cap = std::max(r.cap, b - a);
        if (off) r.cap_bytes = std::max(r.cap_bytes, off[b] - off[a]);
    }
    return r;
}

// for record i, the first byte of its round: what an offset into the records becomes relative to the round's staged block when this is subtracted
inline std::vector<uint64_t> round_bases(const std::vector<uint64_t>& chunk_at, const uint64_t* off) {
    std::vector<uint64_t> base(chunk_at.back());
    for (size_t c = 0; c + 1 < chunk_at.size(); ++c)
        for (uint64_t i = chunk_at[c]; i < chunk_at[c + 1]; ++i) base[i] = off[chunk_at[c]];
    return base;
}

// n + 1 byte offsets of n records: they start at 0 and never step back
inline bool offsets_ok(const uint64_t* off, uint64_t n) {
    if (off[0] != 0) return false;
    for (uint64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

// n rows in launches of at most max_rows rows, blocks of `block` threads: launch(off, m, grid) enqueues rows [off, off + m) on `grid` blocks and
// answers BZK_OK (0) or the status that ends the call
template <class F>
int32_t launch_rows(uint64_t n, uint64_t max_rows, unsigned block, F&& launch) {
    for (uint64_t off = 0; off < n; off += max_rows) {
        const uint64_t m = std::min(n - off, max_rows);
        if (const int32_t s = launch(off, m, (unsigned)((m + block - 1) / block))) return s;
    }
    return 0;
}

}  // namespace bzk
