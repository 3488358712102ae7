// Stand-alone harness of the staging loop of the host-pointer batch calls (bazuka_amd/csrc/bzk_stage.h Stage, bzk_rounds.h round_bases): built with
// the address and undefined-behaviour sanitizers (host code only) and run by tests/test_stage_cpu.py as a child process.  The device operations are
// memcpy / memset on heap blocks of exactly the declared sizes (WsLayout::bind_each), so the sanitizer sees any copy past a buffer's end; the
// "kernel" is a host lambda that derives each output row from that row's staged inputs.  The round boundaries are cut_rounds' own, called here
// directly (tests/host/rounds_check.hip checks them).  The sizes and weights are rounds_check's; three column sets; then every operation of one
// three-round call is made to fail in turn.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../bazuka_amd/csrc/bzk_stage.h"

using namespace bzk;

static int n_cases = 0;
static char what[128];

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            fprintf(stderr, "stage_check: %s: line %d: %s fails\n", what, __LINE__, #cond);    \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

// every operation in order: u(p), d(own), z(ero), s(ync), k(ernel: the caller's lambda); operation number fail_at does nothing and fails
struct Log {
    std::string ops;
    long fail_at = -1;
    int32_t step(char c) {
        ops += c;
        return (long)ops.size() - 1 == fail_at ? BZK_E_DEVICE : BZK_OK;
    }
};
struct HostOps {
    Log* log;
    int32_t up(void* dev, const void* host, size_t bytes) const {
        if (const int32_t s = log->step('u')) return s;
        memcpy(dev, host, bytes);
        return BZK_OK;
    }
    int32_t down(void* host, const void* dev, size_t bytes) const {
        if (const int32_t s = log->step('d')) return s;
        memcpy(host, dev, bytes);
        return BZK_OK;
    }
    int32_t zero(void* dev, size_t bytes) const {
        if (const int32_t s = log->step('z')) return s;
        memset(dev, 0, bytes);
        return BZK_OK;
    }
    int32_t sync() const { return log->step('s'); }
};
// a heap block of its own for every declared buffer, filled with a pattern that is not zero
struct Blocks {
    std::vector<uint8_t*> all;
    void bind(WsLayout& ws) {
        CHECK(ws.ok());
        ws.bind_each([&](size_t bytes) {
            all.push_back(new uint8_t[bytes]);
            memset(all.back(), 0xAA, bytes);
            return all.back();
        });
    }
    ~Blocks() {
        for (uint8_t* p : all) delete[] p;
    }
};
static bool all_zero(const uint8_t* p, size_t bytes) {
    for (size_t i = 0; i < bytes; ++i)
        if (p[i]) return false;
    return true;
}
static uint64_t load64(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}
static uint64_t lcg = 20240901;
static uint64_t next() {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return lcg >> 11;
}
// a weighted sum that tells a byte's place as well as its value
static uint64_t digest(const uint8_t* p, uint64_t len) {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (uint64_t i = 0; i < len; ++i) s = s * 31 + p[i] + 1;
    return s;
}
struct Result {
    int32_t rc;
    std::string ops;
    bool wiped;
};
static std::vector<uint64_t> prefix_sums(const std::vector<uint64_t>& w, uint64_t each) {
    std::vector<uint64_t> off(w.size() + 1, 0);
    for (size_t i = 0; i < w.size(); ++i) off[i + 1] = off[i] + each + w[i];
    return off;
}
// what run() has to have done for the rounds `at`: per round `ups` uploads (and the byte column's where off says the round has bytes), the lambda,
// `downs` downloads; then the overwrites and one synchronise
static std::string expected_ops(const std::vector<uint64_t>& at, const uint64_t* off, int ups, int downs, int wipes) {
    std::string s;
    for (size_t c = 0; c + 1 < at.size(); ++c) {
        if (off && off[at[c + 1]] != off[at[c]]) s += 'u';
        s += std::string(ups, 'u') + 'k' + std::string(downs, 'd');
    }
    return s + std::string(wipes, 'z') + 's';
}

// two fixed inputs (8 and 3 bytes a record), an output (8) and an optional output (2); the first input counts as a secret
static Result fixed_set(const std::vector<uint64_t>& w, bool with_opt, long fail_at) {
    const uint64_t n = w.size();
    std::vector<uint64_t> x(n), z(n, 7);
    std::vector<uint8_t> y(3 * n);
    std::vector<uint16_t> v(n, 7);
    for (uint64_t& e : x) e = next();
    for (uint8_t& e : y) e = (uint8_t)next();
    Log log;
    log.fail_at = fail_at;
    Blocks blocks;
    Stage<HostOps> st({&log}, what, n, 4, 100, [&](uint64_t i) { return w[i]; }, nullptr);
    const std::vector<uint64_t> at = cut_rounds(n, 4, 100, [&](uint64_t i) { return w[i]; });
    CHECK(st.round_at == at && st.cap == round_caps(at, nullptr).cap && st.cap_bytes == 0);
    uint8_t *dx, *dy, *dz, *dv;
    st.in(dx, x.data(), 8); st.in(dy, y.data(), 3); st.out(dz, z.data(), 8); st.out(dv, with_opt ? v.data() : nullptr, 2);
    st.wipe(dx, st.cap * 8);
    blocks.bind(st.ws);
    CHECK(dv != nullptr);  // the buffer exists whether or not it is copied back
    const auto row = [&](uint64_t xi, const uint8_t* yi) { return xi * 3 + digest(yi, 3); };
    uint64_t next_a = 0;
    const int32_t rc = st.run([&](uint64_t a, uint64_t m) {
        if (const int32_t s = log.step('k')) return s;
        CHECK(a == next_a && m >= 1 && m <= st.cap);
        next_a = a + m;
        for (uint64_t j = 0; j < m; ++j) {
            const uint64_t r = row(load64(dx + 8 * j), dy + 3 * j);
            const uint16_t r2 = (uint16_t)(r >> 7);
            memcpy(dz + 8 * j, &r, 8);
            memcpy(dv + 2 * j, &r2, 2);
        }
        return (int32_t)BZK_OK;
    });
    const bool wiped = all_zero(dx, st.cap * 8);
    if (rc != BZK_OK) return {rc, log.ops, wiped};
    CHECK(next_a == n && wiped);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t r = row(x[i], &y[3 * i]);
        CHECK(z[i] == r);
        CHECK(v[i] == (with_opt ? (uint16_t)(r >> 7) : 7));
    }
    CHECK(log.ops == expected_ops(at, nullptr, 2, with_opt ? 2 : 1, 1));  // an absent output costs no operation
    ++n_cases;
    return {rc, log.ops, wiped};
}

// the byte column with its (m + 1) offsets and a padding of 8, as the sha3 / sha512 / keys calls have them: message i is w[i] bytes long and the
// kernel finds it at offsets[j] - off[a], the base it is given
static Result bytes_set(const std::vector<uint64_t>& w, long fail_at) {
    const uint64_t n = w.size();
    const std::vector<uint64_t> off = prefix_sums(w, 0);
    std::vector<uint8_t> data(off[n] + 1);
    for (uint8_t& e : data) e = (uint8_t)next();
    std::vector<uint64_t> out(n, 7);
    Log log;
    log.fail_at = fail_at;
    Blocks blocks;
    Stage<HostOps> st({&log}, what, n, 4, 100, lengths(off.data()), off.data());
    const std::vector<uint64_t> at = cut_rounds(n, 4, 100, lengths(off.data()));
    const RoundCaps caps = round_caps(at, off.data());
    CHECK(st.round_at == at && st.cap == caps.cap && st.cap_bytes == caps.cap_bytes);
    uint8_t *ddata, *doff, *dout;
    st.bytes(ddata, data.data(), 0, 8); st.offsets(doff); st.out(dout, out.data(), 8);
    st.wipe(ddata, st.cap_bytes + 8); st.wipe(dout, st.cap * 8);  // as the keys calls: seeds and keys
    blocks.bind(st.ws);
    const int32_t rc = st.run([&](uint64_t a, uint64_t m) {
        if (const int32_t s = log.step('k')) return s;
        for (uint64_t j = 0; j < m; ++j) {
            const uint64_t b = load64(doff + 8 * j) - off[a], e = load64(doff + 8 * (j + 1)) - off[a];
            CHECK(b <= e && e <= st.cap_bytes);
            const uint64_t r = digest(ddata + b, e - b);
            memcpy(dout + 8 * j, &r, 8);
        }
        return (int32_t)BZK_OK;
    });
    const bool wiped = all_zero(ddata, st.cap_bytes + 8) && all_zero(dout, st.cap * 8);
    if (rc != BZK_OK) return {rc, log.ops, wiped};
    CHECK(wiped);
    for (uint64_t i = 0; i < n; ++i) CHECK(out[i] == digest(&data[off[i]], w[i]));
    CHECK(log.ops == expected_ops(at, off.data(), 1, 1, 2));
    ++n_cases;
    return {rc, log.ops, wiped};
}

// Records of a 5-byte header and a payment of w[i] bytes, staged as they stand behind a 16-byte prefix; the rounds are cut by the payments' lengths
// and the kernel reads payment i at begin[i] .. end[i], relative to its round's first byte, as the withdraw runs build them (the prefix and its
// overwrite are l1_txs_sign_run's).  A fixed column of "keys" rides along and is overwritten too.
static Result relative_set(const std::vector<uint64_t>& w, long fail_at) {
    const uint64_t n = w.size(), HDR = 5, PREFIX = 16;
    const std::vector<uint64_t> rec_off = prefix_sums(w, HDR);
    std::vector<uint8_t> txs(rec_off[n] + 1);
    for (uint8_t& e : txs) e = (uint8_t)next();
    std::vector<uint64_t> keys(n), out(n, 7);
    for (uint64_t& e : keys) e = next();
    Log log;
    log.fail_at = fail_at;
    Blocks blocks;
    Stage<HostOps> st({&log}, what, n, 4, 100, [&](uint64_t i) { return w[i]; }, rec_off.data());
    const std::vector<uint64_t> at = cut_rounds(n, 4, 100, [&](uint64_t i) { return w[i]; });
    const RoundCaps caps = round_caps(at, rec_off.data());
    CHECK(st.round_at == at && st.cap == caps.cap && st.cap_bytes == caps.cap_bytes);
    std::vector<uint64_t> begin = round_bases(st.round_at, rec_off.data()), end(n);
    for (size_t c = 0; c + 1 < at.size(); ++c)
        for (uint64_t i = at[c]; i < at[c + 1]; ++i) CHECK(begin[i] == rec_off[at[c]]);
    for (uint64_t i = 0; i < n; ++i) {
        begin[i] = rec_off[i] + HDR - begin[i];
        end[i] = begin[i] + w[i];
    }
    uint8_t *dbytes, *dbeg, *dend, *dkeys, *dout;
    st.bytes(dbytes, txs.data(), PREFIX, 0); st.in(dbeg, begin.data(), 8); st.in(dend, end.data(), 8); st.in(dkeys, keys.data(), 8);
    st.out(dout, out.data(), 8);
    st.wipe(dkeys, st.cap * 8); st.wipe(dbytes, PREFIX);
    blocks.bind(st.ws);
    const int32_t rc = st.run([&](uint64_t a, uint64_t m) {
        if (const int32_t s = log.step('k')) return s;
        memset(dbytes, 0x5C, PREFIX);  // the lanes' own secrets
        for (uint64_t j = 0; j < m; ++j) {
            const uint64_t b = load64(dbeg + 8 * j), e = load64(dend + 8 * j);
            CHECK(e - b == w[a + j] && e <= st.cap_bytes);
            CHECK(memcmp(dbytes + PREFIX + b, &txs[rec_off[a + j] + HDR], e - b) == 0);  // the record's bytes lie at begin[i] of the staged block
            const uint64_t r = digest(dbytes + PREFIX + b, e - b) ^ load64(dkeys + 8 * j);
            memcpy(dout + 8 * j, &r, 8);
        }
        return (int32_t)BZK_OK;
    });
    const bool wiped = all_zero(dkeys, st.cap * 8) && all_zero(dbytes, PREFIX);
    if (rc != BZK_OK) return {rc, log.ops, wiped};
    CHECK(wiped);
    for (uint64_t i = 0; i < n; ++i) CHECK(out[i] == (digest(&txs[rec_off[i] + HDR], w[i]) ^ keys[i]));
    CHECK(log.ops == expected_ops(at, rec_off.data(), 3, 1, 2));
    ++n_cases;
    return {rc, log.ops, wiped};
}

static void all_sets(const std::vector<uint64_t>& w) {
    CHECK(fixed_set(w, true, -1).rc == BZK_OK);
    CHECK(fixed_set(w, false, -1).rc == BZK_OK);
    CHECK(bytes_set(w, -1).rc == BZK_OK);
    CHECK(relative_set(w, -1).rc == BZK_OK);
}

// every operation of one call fails in turn: the status is BZK_E_DEVICE, what ran before it is the good run's, nothing follows it but the `wipes`
// overwrites and their synchronise, and every registered region is zero
template <class F>
static void early_exits(const char* name, int wipes, F run) {
    snprintf(what, sizeof what, "%s, no failure", name);
    const Result good = run(-1);
    CHECK(good.rc == BZK_OK);
    const std::string tail = std::string(wipes, 'z') + 's';
    for (long k = 0; k < (long)good.ops.size(); ++k) {
        snprintf(what, sizeof what, "%s, operation %ld of %zu fails", name, k, good.ops.size());
        const Result r = run(k);
        CHECK(r.rc == BZK_E_DEVICE);
        CHECK(r.ops == good.ops.substr(0, k + 1) + tail);
        CHECK(r.wiped);
        ++n_cases;
    }
}

int main() {
    const uint64_t sizes[] = {0, 1, 2, 3, 4, 5, 8, 9};
    for (uint64_t n : sizes) {
        for (uint64_t flat : {0, 25, 26}) {  // 25: four records fit exactly
            snprintf(what, sizeof what, "n = %llu, every weight %llu", (unsigned long long)n, (unsigned long long)flat);
            all_sets(std::vector<uint64_t>(n, flat));
        }
        for (int place = 0; place < 3 && n; ++place) {  // one record over the weight limit: first, middle, last
            std::vector<uint64_t> w(n, 10);
            const uint64_t k = place == 0 ? 0 : place == 1 ? n / 2 : n - 1;
            w[k] = 101;
            snprintf(what, sizeof what, "n = %llu, weight 101 at %llu", (unsigned long long)n, (unsigned long long)k);
            all_sets(w);
        }
        for (int rep = 0; rep < 16; ++rep) {
            std::vector<uint64_t> w(n);
            for (uint64_t& x : w) x = next() % 121;
            snprintf(what, sizeof what, "n = %llu, random mix %d", (unsigned long long)n, rep);
            all_sets(w);
        }
    }
    const std::vector<uint64_t> three_rounds(9, 10);  // 4 + 4 + 1 records
    CHECK(cut_rounds(9, 4, 100, [](uint64_t) { return (uint64_t)10; }).size() == 4);
    early_exits("relative set, 9 records", 2, [&](long k) { return relative_set(three_rounds, k); });
    early_exits("byte column, 9 records", 2, [&](long k) { return bytes_set(three_rounds, k); });
    early_exits("fixed set, 9 records", 1, [&](long k) { return fixed_set(three_rounds, true, k); });
    printf("stage_check: %d cases hold\n", n_cases);
    return 0;
}
