// Stand-alone harness of the staging-round cutter (bazuka_amd/csrc/bzk_rounds.h cut_rounds, round_caps): built with the address and
// undefined-behaviour sanitizers (host code only) and run by tests/test_rounds_cpu.py as a child process.  Every case asserts the cutter's rules
// directly - the rounds partition [0, n) in order, each holds a record, none holds more than max_records, one is over max_weight only when it
// holds exactly one record, each is maximal, and cap / cap_bytes are the maxima over the rounds - on a grid of small limits, then two cases at
// the shipped limits with fixed expectations.
#include <stdio.h>
#include <stdlib.h>

#include "../../bazuka_amd/csrc/bzk_rounds.h"

using namespace bzk;

static int n_cases = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "rounds_check: %s: %s fails\n", what, #cond);            \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

// the rules, for weights w (n of them) under the two limits; returns the round starts
static std::vector<uint64_t> check_case(const char* what, const std::vector<uint64_t>& w, uint64_t max_records, uint64_t max_weight) {
    const uint64_t n = w.size();
    const std::vector<uint64_t> at = cut_rounds(n, max_records, max_weight, [&](uint64_t i) { return w[i]; });
    CHECK(!at.empty() && at.front() == 0 && at.back() == n);
    CHECK(n != 0 || at.size() == 1);
    std::vector<uint64_t> off(n + 1, 0);  // the offsets whose differences are the weights
    for (uint64_t i = 0; i < n; ++i) off[i + 1] = off[i] + w[i];
    uint64_t cap = 0, cap_bytes = 0;
    for (size_t c = 0; c + 1 < at.size(); ++c) {
        const uint64_t a = at[c], b = at[c + 1];
        CHECK(a < b && b <= n);            // in order, at least one record
        CHECK(b - a <= max_records);
        const uint64_t sum = off[b] - off[a];
        CHECK(sum <= max_weight || b - a == 1);
        if (b < n) CHECK(b - a == max_records || sum > max_weight || w[b] > max_weight - sum);  // maximal: record b would have broken a limit
        cap = cap > b - a ? cap : b - a;
        cap_bytes = cap_bytes > sum ? cap_bytes : sum;
    }
    const RoundCaps rc = round_caps(at, off.data());
    CHECK(rc.cap == cap && rc.cap_bytes == cap_bytes);
    ++n_cases;
    return at;
}

int main() {
    const uint64_t sizes[] = {0, 1, 2, 3, 4, 5, 8, 9};
    uint64_t lcg = 20240901;  // the seeded mix
    for (uint64_t n : sizes) {
        char what[96];
        for (uint64_t flat : {0, 25, 26}) {  // 25: four records fit exactly
            snprintf(what, sizeof what, "n = %llu, every weight %llu", (unsigned long long)n, (unsigned long long)flat);
            check_case(what, std::vector<uint64_t>(n, flat), 4, 100);
        }
        for (int place = 0; place < 3 && n; ++place) {  // one record over the weight limit: first, middle, last
            std::vector<uint64_t> w(n, 10);
            const uint64_t k = place == 0 ? 0 : place == 1 ? n / 2 : n - 1;
            w[k] = 101;
            snprintf(what, sizeof what, "n = %llu, weight 101 at %llu", (unsigned long long)n, (unsigned long long)k);
            const std::vector<uint64_t> at = check_case(what, w, 4, 100);
            bool alone = false;
            for (size_t c = 0; c + 1 < at.size(); ++c) alone = alone || (at[c] == k && at[c + 1] == k + 1);
            CHECK(alone);
        }
        for (int rep = 0; rep < 16; ++rep) {
            std::vector<uint64_t> w(n);
            for (uint64_t& x : w) {
                lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
                x = (lcg >> 33) % 121;
            }
            snprintf(what, sizeof what, "n = %llu, random mix %d", (unsigned long long)n, rep);
            check_case(what, w, 4, 100);
        }
    }
    {  // sums that would wrap a 64-bit addition
        const char* what = "weights near 2^64";
        const std::vector<uint64_t> at = check_case(what, {~(uint64_t)0, ~(uint64_t)0 - 5, 3, 4}, 4, ~(uint64_t)0 - 1);
        CHECK((at == std::vector<uint64_t>{0, 1, 3, 4}));
    }
    {  // the record limit of the shipped paths
        const char* what = "70 000 records of 111 bytes";
        const std::vector<uint64_t> at = check_case(what, std::vector<uint64_t>(70000, 111), (uint64_t)1 << 16, (uint64_t)64 << 20);
        CHECK((at == std::vector<uint64_t>{0, 65536, 70000}));
    }
    {  // the byte limit: 1 115 x 60 144 = 67 060 560 <= 67 108 864 < 1 116 x 60 144
        const char* what = "1 150 records of 60 144 bytes";
        const std::vector<uint64_t> at = check_case(what, std::vector<uint64_t>(1150, 60144), (uint64_t)1 << 16, (uint64_t)64 << 20);
        CHECK((at == std::vector<uint64_t>{0, 1115, 1150}));
    }
    printf("rounds_check: %d cases hold\n", n_cases);
    return 0;
}
