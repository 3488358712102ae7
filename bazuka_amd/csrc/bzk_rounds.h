// Staging rounds of a batched call: which records go up together.  Index arithmetic only, plain C++ (checked stand-alone by
// tests/host/rounds_check.hip); the per-round relative offsets and everything a round launches stay with the callers (eddsa.hip).
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

// what the longest round needs: cap records, and cap_bytes = the largest off[b] - off[a] over the rounds [a, b) (off: n + 1 byte offsets)
struct RoundCaps {
    uint64_t cap = 0, cap_bytes = 0;
};
inline RoundCaps round_caps(const std::vector<uint64_t>& chunk_at, const uint64_t* off) {
    RoundCaps r;
    for (size_t c = 0; c + 1 < chunk_at.size(); ++c) {
        const uint64_t a = chunk_at[c], b = chunk_at[c + 1];
        r.cap = std::max(r.cap, b - a);
        r.cap_bytes = std::max(r.cap_bytes, off[b] - off[a]);
    }
    return r;
}

}  // namespace bzk
