// Reader / writer for bellman's `groth16::Parameters<Bls12>` byte format - the proving-key files real networks ship
// (VERDICT r1 item 8).  Host code only.
//
// The reference never touches this format itself: its external prover does (README.md:26-28; the dev network generates its
// keys in memory, src/config/blockchain.rs:355-417).  bellman = "0.14.0" and bls12_381 = "0.8.0" are un-vendored
// (Cargo.toml:29-30), so the layout is restated from the published crates [recalled]:
//   Parameters::write  = VerifyingKey::write | u32-BE len(h) | h.. | u32-BE len(l) | l.. | u32-BE len(a) | a.. |
//                        u32-BE len(b_g1) | b_g1.. | u32-BE len(b_g2) | b_g2..
//   VerifyingKey::write = alpha_g1 | beta_g1 | beta_g2 | gamma_g2 | delta_g1 | delta_g2 | u32-BE len(ic) | ic..
//   G1Affine::to_uncompressed = x | y, 48-byte BIG-endian canonical integers; G2Affine = x.c1 | x.c0 | y.c1 | y.c0;
//   flag bits of byte 0: 0x80 compressed (must be clear here), 0x40 point at infinity (all other bits zero), 0x20 sort flag
//   (compressed form only, must be clear).
// Parameters::read refuses the point at infinity inside h / l / a / b_g1 / b_g2, and so does this reader.  Points are checked
// to be canonical (< p) and on the curve, which is `read(.., checked = false)`.  The subgroup check of `checked = true` is no part
// of decode or of bzk_params_load_bellman: bzk_bellman_params_check and bzk_params_load_bellman_checked below add it, through the
// per-point functions of subgroup.hip (the queries on the device, the verifying key and ic on the host).
// In memory everything is the reference's own raw form: little-endian Montgomery limbs (src/zk/groth16/mod.rs:19-38).
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "bzk_curve.cuh"
#include "bzk_internal.h"
#include "bzk_rekey.h"

using namespace bzk;

namespace {

bool fp_from_be(const uint8_t* be, uint8_t flags_mask, Fp& out) {  // canonical big-endian -> Montgomery; false when >= p
    Fp c;
    for (int w = 0; w < 12; ++w) {
        const uint8_t* b = be + 44 - 4 * w;
        uint32_t v = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
        if (w == 11) v &= ~((uint32_t)flags_mask << 24);
        c.l[w] = v;
    }
    Fp t = c;
    uint64_t borrow = 0;
    for (int i = 0; i < 12; ++i) {
        uint64_t d = (uint64_t)t.l[i] - FpParams::MOD[i] - borrow;
        borrow = (d >> 63) & 1;
    }
    if (!borrow) return false;  // c >= p
    out = fe_to_mont<FpParams>(c);
    return true;
}
void fp_to_be(const Fp& mont, uint8_t* be) {
    const Fp c = fe_from_mont<FpParams>(mont);
    for (int w = 0; w < 12; ++w) {
        uint8_t* b = be + 44 - 4 * w;
        b[0] = (uint8_t)(c.l[w] >> 24); b[1] = (uint8_t)(c.l[w] >> 16); b[2] = (uint8_t)(c.l[w] >> 8); b[3] = (uint8_t)c.l[w];
    }
}
Fp fp_b4() {  // 4 in Montgomery form
    Fp c = Fp::zero();
    c.l[0] = 4;
    return fe_to_mont<FpParams>(c);
}

// 1 = a finite point on the curve, 2 = the point at infinity, 0 = malformed
int g1_decode(const uint8_t* in, uint8_t* raw96) {
    const uint8_t fl = in[0] & 0xe0;
    if (fl & 0x80 || fl & 0x20) return 0;
    if (fl & 0x40) {
        if (in[0] != 0x40) return 0;
        for (int i = 1; i < 96; ++i) if (in[i]) return 0;
        return 2;
    }
    Fp x, y;
    if (!fp_from_be(in, 0xe0, x) || !fp_from_be(in + 48, 0, y)) return 0;
    const Fp lhs = fe_sqr<FpParams>(y), rhs = fe_add<FpParams>(fe_mul<FpParams>(fe_sqr<FpParams>(x), x), fp_b4());
    if (!lhs.equals(rhs)) return 0;
    memcpy(raw96, x.l, 48);
    memcpy(raw96 + 48, y.l, 48);
    return 1;
}
int g2_decode(const uint8_t* in, uint8_t* raw192) {
    const uint8_t fl = in[0] & 0xe0;
    if (fl & 0x80 || fl & 0x20) return 0;
    if (fl & 0x40) {
        if (in[0] != 0x40) return 0;
        for (int i = 1; i < 192; ++i) if (in[i]) return 0;
        return 2;
    }
    Fp2 x, y;
    if (!fp_from_be(in, 0xe0, x.c1) || !fp_from_be(in + 48, 0, x.c0) || !fp_from_be(in + 96, 0, y.c1) || !fp_from_be(in + 144, 0, y.c0)) return 0;
    const Fp2 b = {fp_b4(), fp_b4()};  // 4 (1 + u)
    const Fp2 lhs = Fp2Ops::sqr(y), rhs = Fp2Ops::add(Fp2Ops::mul(Fp2Ops::sqr(x), x), b);
    if (!Fp2Ops::eq(lhs, rhs)) return 0;
    memcpy(raw192, x.c0.l, 48); memcpy(raw192 + 48, x.c1.l, 48); memcpy(raw192 + 96, y.c0.l, 48); memcpy(raw192 + 144, y.c1.l, 48);
    return 1;
}
void g1_encode(const uint8_t* raw96, bool inf, uint8_t* out) {
    if (inf) { memset(out, 0, 96); out[0] = 0x40; return; }
    Fp x, y;
    memcpy(x.l, raw96, 48); memcpy(y.l, raw96 + 48, 48);
    fp_to_be(x, out); fp_to_be(y, out + 48);
}
void g2_encode(const uint8_t* raw192, bool inf, uint8_t* out) {
    if (inf) { memset(out, 0, 192); out[0] = 0x40; return; }
    Fp f[4];
    for (int i = 0; i < 4; ++i) memcpy(f[i].l, raw192 + 48 * i, 48);
    fp_to_be(f[1], out); fp_to_be(f[0], out + 48); fp_to_be(f[3], out + 96); fp_to_be(f[2], out + 144);
}
uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

struct Layout {  // byte offsets of the seven arrays inside a Parameters blob
    uint64_t n_ic, n_h, n_l, n_a, n_b1, n_b2;
    uint64_t off_ic, off_h, off_l, off_a, off_b1, off_b2, total;
};
constexpr uint64_t VK_HEAD = 3 * 96 + 3 * 192;  // alpha_g1, beta_g1, delta_g1; beta_g2, gamma_g2, delta_g2
bool layout_of(const uint8_t* b, uint64_t len, Layout& L) {
    uint64_t p = VK_HEAD;
    auto count = [&](uint64_t& n, uint64_t& off, uint64_t sz) {
        if (p + 4 > len) return false;
        n = be32(b + p);
        p += 4;
        off = p;
        if (n > (len - p) / sz) return false;
        p += n * sz;
        return true;
    };
    if (len < VK_HEAD) return false;
    if (!count(L.n_ic, L.off_ic, 96) || !count(L.n_h, L.off_h, 96) || !count(L.n_l, L.off_l, 96) || !count(L.n_a, L.off_a, 96) ||
        !count(L.n_b1, L.off_b1, 96) || !count(L.n_b2, L.off_b2, 192))
        return false;
    L.total = p;
    return true;
}
template <class Fn>
bool parallel_points(uint64_t n, int threads, Fn&& one) {  // one(i) -> ok
    if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
    threads = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)threads, n / 4096 + 1));
    std::atomic<bool> ok{true};
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            for (uint64_t i = (uint64_t)t; i < n && ok.load(std::memory_order_relaxed); i += (uint64_t)threads)
                if (!one(i)) ok.store(false);
        });
    for (auto& x : th) x.join();
    return ok.load();
}

// ---- the checked reader: where the first failure is, in file order
const char* const ARRAY_NAME[8] = {"the verifying key", "ic", "h", "l", "a", "b_g1", "b_g2", "the array lengths"};
struct Decoded {
    Layout L;
    std::vector<uint8_t> vk, ic, h, l, a, b1, b2;
};
struct HeadPoint { uint64_t src, dst; bool g2; };  // file offset, offset in vk870
const HeadPoint HEAD[6] = {{0, 0, false}, {96, 97, false}, {192, 194, true}, {384, 387, true}, {576, 580, false}, {672, 677, true}};
bool fail_at(uint64_t report[4], uint64_t array, uint64_t index, uint64_t code) {
    report[0] = array; report[1] = index; report[2] = code; report[3] = 0;
    return false;
}
// bzk_bellman_params_decode into D; when it refuses, a second, sequential pass names the record (a refusal is the rare path)
bool decode_located(const uint8_t* bytes, uint64_t len, Decoded& D, uint64_t report[4]) {
    Layout& L = D.L;
    if (!layout_of(bytes, len, L)) return fail_at(report, 7, 0, 2);
    D.vk.resize(870); D.ic.resize(97 * L.n_ic); D.h.resize(96 * L.n_h); D.l.resize(96 * L.n_l); D.a.resize(96 * L.n_a);
    D.b1.resize(96 * L.n_b1); D.b2.resize(192 * L.n_b2);
    if (bzk_bellman_params_decode(bytes, len, D.vk.data(), D.ic.data(), D.h.data(), D.l.data(), D.a.data(), D.b1.data(), D.b2.data(), 0) == BZK_OK)
        return true;
    uint8_t raw[192];
    for (uint64_t k = 0; k < 6; ++k)
        if (!(HEAD[k].g2 ? g2_decode(bytes + HEAD[k].src, raw) : g1_decode(bytes + HEAD[k].src, raw))) return fail_at(report, 0, k, 2);
    for (uint64_t i = 0; i < L.n_ic; ++i)
        if (!g1_decode(bytes + L.off_ic + 96 * i, raw)) return fail_at(report, 1, i, 2);
    const uint64_t off[4] = {L.off_h, L.off_l, L.off_a, L.off_b1}, cnt[4] = {L.n_h, L.n_l, L.n_a, L.n_b1};
    for (int q = 0; q < 4; ++q)
        for (uint64_t i = 0; i < cnt[q]; ++i)
            if (g1_decode(bytes + off[q] + 96 * i, raw) != 1) return fail_at(report, 2 + q, i, 2);  // malformed, off the curve, or the identity inside a query
    for (uint64_t i = 0; i < L.n_b2; ++i)
        if (g2_decode(bytes + L.off_b2 + 192 * i, raw) != 1) return fail_at(report, 6, i, 2);
    return fail_at(report, 7, 0, 2);
}
// the six verifying-key points and ic on the host (a handful of points); the identity passes, as it does in the decoder
bool head_in_subgroup(const Decoded& D, uint64_t report[4]) {
    for (uint64_t k = 0; k < 6; ++k) {
        const uint8_t* p = D.vk.data() + HEAD[k].dst;
        if (p[HEAD[k].g2 ? 192 : 96]) continue;
        const uint8_t v = sg_host_one(HEAD[k].g2, p);
        if (v != 1) return fail_at(report, 0, k, v);
    }
    for (uint64_t i = 0; i < D.L.n_ic; ++i) {
        const uint8_t* p = D.ic.data() + 97 * i;
        if (p[96]) continue;
        const uint8_t v = sg_host_one(false, p);
        if (v != 1) return fail_at(report, 1, i, v);
    }
    return true;
}
// the five queries in file order: q[k] = h, l, a, b_g1, b_g2 as raw records, in host memory or (on_device) where bzk_params_load put them.
// *pass = false and report filled at the first failure
int32_t queries_in_subgroup(bzk_ctx* ctx, const char* who, const uint8_t* const q[5], bool on_device, const Layout& L, uint64_t report[4], bool* pass) {
    const uint64_t cnt[5] = {L.n_h, L.n_l, L.n_a, L.n_b1, L.n_b2};
    *pass = true;
    for (int k = 0; k < 5; ++k) {
        uint64_t idx = 0;
        uint8_t code = 1;
        const int32_t st = sg_first_bad(ctx, who, k == 4, q[k], on_device, cnt[k], &idx, &code);
        if (st != BZK_OK) return st;
        if (idx < cnt[k]) {
            *pass = fail_at(report, 2 + k, idx, code);
            return BZK_OK;
        }
    }
    return BZK_OK;
}
std::string failure_text(const uint64_t report[4]) {
    static const char* const WHAT[3] = {"is on the curve but outside the order-r subgroup", "", "is malformed, off the curve, or the point at infinity inside a query"};
    if (report[0] >= 7) return "bellman parameters: truncated or malformed";
    return std::string("bellman parameters: ") + ARRAY_NAME[report[0]] + "[" + std::to_string(report[1]) + "] " + WHAT[report[2] == 0 ? 0 : 2];
}

}  // namespace

extern "C" {

// info = len(ic), len(h), len(l), len(a), len(b_g1), len(b_g2), bytes consumed
int32_t bzk_bellman_params_info(const uint8_t* bytes, uint64_t len, uint64_t info[7]) {
    Layout L;
    if (!bytes || !info || !layout_of(bytes, len, L)) return BZK_E_ARG;
    info[0] = L.n_ic; info[1] = L.n_h; info[2] = L.n_l; info[3] = L.n_a; info[4] = L.n_b1; info[5] = L.n_b2; info[6] = L.total;
    return BZK_OK;
}

// vk870 = alpha_g1 | beta_g1 | beta_g2 | gamma_g2 | delta_g1 | delta_g2 as packed 97 / 193-byte points (the head of
// `Groth16VerifyingKey`, src/zk/groth16/mod.rs:22-31); ic = n_ic packed 97-byte points; h, l, a, b_g1 raw 96 B; b_g2 raw 192 B.
int32_t bzk_bellman_params_decode(const uint8_t* bytes, uint64_t len, uint8_t* vk870, uint8_t* ic, uint8_t* h, uint8_t* l, uint8_t* a,
                                  uint8_t* b_g1, uint8_t* b_g2, int32_t threads) {
    Layout L;
    if (!bytes || !vk870 || !layout_of(bytes, len, L)) return BZK_E_ARG;
    if ((L.n_ic && !ic) || (L.n_h && !h) || (L.n_l && !l) || (L.n_a && !a) || (L.n_b1 && !b_g1) || (L.n_b2 && !b_g2)) return BZK_E_ARG;
    // verifying key: infinity is representable here (packed form carries the flag byte)
    auto vk_g1 = [&](uint64_t src, uint64_t dst) {
        uint8_t raw[96] = {0};
        const int k = g1_decode(bytes + src, raw);
        if (!k) return false;
        memcpy(vk870 + dst, raw, 96);
        if (k == 2) { memset(vk870 + dst, 0, 96); Fp one = Fp::one(); memcpy(vk870 + dst + 48, one.l, 48); }  // bls12_381 identity: (0, 1, inf)
        vk870[dst + 96] = k == 2;
        return true;
    };
    auto vk_g2 = [&](uint64_t src, uint64_t dst) {
        uint8_t raw[192] = {0};
        const int k = g2_decode(bytes + src, raw);
        if (!k) return false;
        memcpy(vk870 + dst, raw, 192);
        if (k == 2) { memset(vk870 + dst, 0, 192); Fp one = Fp::one(); memcpy(vk870 + dst + 96, one.l, 48); }
        vk870[dst + 192] = k == 2;
        return true;
    };
    // file order: alpha_g1, beta_g1, beta_g2, gamma_g2, delta_g1, delta_g2 = the packed order
    if (!vk_g1(0, 0) || !vk_g1(96, 97) || !vk_g2(192, 194) || !vk_g2(384, 387) || !vk_g1(576, 580) || !vk_g2(672, 677)) return BZK_E_ARG;
    for (uint64_t i = 0; i < L.n_ic; ++i) {
        uint8_t raw[96] = {0};
        const int k = g1_decode(bytes + L.off_ic + 96 * i, raw);
        if (!k) return BZK_E_ARG;
        if (k == 2) { memset(raw, 0, 96); Fp one = Fp::one(); memcpy(raw + 48, one.l, 48); }
        memcpy(ic + 97 * i, raw, 96);
        ic[97 * i + 96] = k == 2;
    }
    // the queries: finite points only (Parameters::read: "point at infinity")
    bool ok = parallel_points(L.n_h, threads, [&](uint64_t i) { return g1_decode(bytes + L.off_h + 96 * i, h + 96 * i) == 1; }) &&
              parallel_points(L.n_l, threads, [&](uint64_t i) { return g1_decode(bytes + L.off_l + 96 * i, l + 96 * i) == 1; }) &&
              parallel_points(L.n_a, threads, [&](uint64_t i) { return g1_decode(bytes + L.off_a + 96 * i, a + 96 * i) == 1; }) &&
              parallel_points(L.n_b1, threads, [&](uint64_t i) { return g1_decode(bytes + L.off_b1 + 96 * i, b_g1 + 96 * i) == 1; }) &&
              parallel_points(L.n_b2, threads, [&](uint64_t i) { return g2_decode(bytes + L.off_b2 + 192 * i, b_g2 + 192 * i) == 1; });
    return ok ? BZK_OK : BZK_E_ARG;
}

// the inverse (`Parameters::write`): out NULL = size query
int32_t bzk_bellman_params_encode(const uint8_t vk870[870], const uint8_t* ic, uint64_t n_ic, const uint8_t* h, uint64_t n_h, const uint8_t* l,
                                  uint64_t n_l, const uint8_t* a, uint64_t n_a, const uint8_t* b_g1, const uint8_t* b_g2, uint64_t n_b,
                                  uint8_t* out, uint64_t cap, uint64_t* size_out) {
    if (!vk870 || (n_ic && !ic) || (n_h && !h) || (n_l && !l) || (n_a && !a) || (n_b && (!b_g1 || !b_g2))) return BZK_E_ARG;
    if ((n_ic | n_h | n_l | n_a | n_b) >> 32) return BZK_E_ARG;
    const uint64_t total = VK_HEAD + 4 + 96 * n_ic + 4 + 96 * n_h + 4 + 96 * n_l + 4 + 96 * n_a + 4 + 96 * n_b + 4 + 192 * n_b;
    if (size_out) *size_out = total;
    if (!out) return BZK_OK;
    if (cap < total) return BZK_E_ARG;
    g1_encode(vk870, vk870[96] != 0, out);
    g1_encode(vk870 + 97, vk870[97 + 96] != 0, out + 96);
    g2_encode(vk870 + 194, vk870[194 + 192] != 0, out + 192);
    g2_encode(vk870 + 387, vk870[387 + 192] != 0, out + 384);
    g1_encode(vk870 + 580, vk870[580 + 96] != 0, out + 576);
    g2_encode(vk870 + 677, vk870[677 + 192] != 0, out + 672);
    uint64_t p = VK_HEAD;
    put32(out + p, (uint32_t)n_ic); p += 4;
    for (uint64_t i = 0; i < n_ic; ++i, p += 96) g1_encode(ic + 97 * i, ic[97 * i + 96] != 0, out + p);
    auto arr = [&](const uint8_t* src, uint64_t n, uint64_t raw, bool g2) {
        put32(out + p, (uint32_t)n);
        p += 4;
        uint8_t* base = out + p;
        parallel_points(n, 0, [&](uint64_t i) {
            if (g2) g2_encode(src + raw * i, false, base + raw * i);
            else g1_encode(src + raw * i, false, base + raw * i);
            return true;
        });
        p += n * raw;
    };
    arr(h, n_h, 96, false); arr(l, n_l, 96, false); arr(a, n_a, 96, false); arr(b_g1, n_b, 96, false); arr(b_g2, n_b, 192, true);
    return BZK_OK;
}

// One call for a prover: parse + upload.  The file does not say WHICH variables the `a` / `b` queries belong to - bellman's
// prover derives that from the circuit (a_aux_density, b_input_density, b_aux_density); the caller passes the density maps of
// the circuit shape (bzk_r1cs_data views 4 and 5 of `MpnCircuit::empty`) and the counts must agree with the file.
// vk_out (optional) receives bincode(Groth16VerifyingKey) = 870 + 8 + 97 n_in bytes, what `MpnWork::vk()` is compared with.
// report = NULL: the unchecked reader.  Otherwise `Parameters::read(.., checked = true)`: the verifying key and ic are checked on the host before anything is
// uploaded, the queries on the device in the arrays bzk_params_load has just uploaded (one upload; a failure frees the handle again)
static int32_t load_bellman(bzk_ctx* ctx, const uint8_t* bytes, uint64_t len, uint32_t n_in, uint32_t n_aux, const uint8_t* a_density,
                            const uint8_t* b_density, bzk_params** out, uint8_t* vk_out, uint64_t vk_cap, uint64_t* report) {
    if (!ctx || !bytes || !out || !a_density || !b_density) return BZK_E_ARG;
    *out = nullptr;
    if (report) report[0] = report[1] = report[2] = report[3] = 0;
    Layout L;
    if (!layout_of(bytes, len, L)) {
        ctx->last_error = "bellman parameters: truncated or malformed";
        if (report) fail_at(report, 7, 0, 2);
        return BZK_E_ARG;
    }
    uint64_t n_a = 0, n_b = 0;
    for (uint64_t i = 0; i < (uint64_t)n_in + n_aux; ++i) { n_a += a_density[i] != 0; n_b += b_density[i] != 0; }
    const uint64_t m = L.n_h + 1;
    uint32_t log_m = 0;
    while (((uint64_t)1 << log_m) < m) ++log_m;
    if (L.n_ic != n_in || L.n_l != n_aux || L.n_a != n_a || L.n_b1 != n_b || L.n_b2 != n_b || ((uint64_t)1 << log_m) != m || log_m > 28) {
        ctx->last_error = "bellman parameters: array lengths do not fit the circuit shape (ic " + std::to_string(L.n_ic) + ", h " + std::to_string(L.n_h) +
                          ", l " + std::to_string(L.n_l) + ", a " + std::to_string(L.n_a) + ", b " + std::to_string(L.n_b1) + "/" + std::to_string(L.n_b2) + ")";
        if (report) fail_at(report, 7, 0, 2);
        return BZK_E_ARG;
    }
    Decoded D;
    if (report) {
        if (!decode_located(bytes, len, D, report) || !head_in_subgroup(D, report)) {
            ctx->last_error = failure_text(report);
            return BZK_E_ARG;
        }
    } else {
        D.vk.resize(870); D.ic.resize(97 * L.n_ic); D.h.resize(96 * L.n_h); D.l.resize(96 * L.n_l); D.a.resize(96 * L.n_a);
        D.b1.resize(96 * L.n_b1); D.b2.resize(192 * L.n_b2);
        if (bzk_bellman_params_decode(bytes, len, D.vk.data(), D.ic.data(), D.h.data(), D.l.data(), D.a.data(), D.b1.data(), D.b2.data(), 0) != BZK_OK) {
            ctx->last_error = "bellman parameters: a point is malformed, not on the curve, or the point at infinity inside a query";
            return BZK_E_ARG;
        }
    }
    if (vk_out) {
        const uint64_t need = 870 + 8 + 97 * L.n_ic;
        if (vk_cap < need) return BZK_E_ARG;
        memcpy(vk_out, D.vk.data(), 870);
        const uint64_t cnt = L.n_ic;
        memcpy(vk_out + 870, &cnt, 8);  // bincode u64 length, little-endian host
        memcpy(vk_out + 878, D.ic.data(), 97 * L.n_ic);
    }
    bzk_params_desc d;
    memset(&d, 0, sizeof d);
    d.n_in = n_in; d.n_aux = n_aux; d.log_m = log_m; d.n_a = (uint32_t)n_a; d.n_b = (uint32_t)n_b;
    d.vk = D.vk.data(); d.h = D.h.data(); d.l = D.l.data(); d.a = D.a.data(); d.b_g1 = D.b1.data(); d.b_g2 = D.b2.data();
    d.a_density = a_density; d.b_density = b_density;
    const int32_t st = bzk_params_load(ctx, &d, out);
    if (st != BZK_OK || !report) return st;
    void* dev[5];
    bzk_params_buffers_internal(*out, &dev[0], &dev[1], &dev[2], &dev[3], &dev[4]);
    const uint8_t* q[5];
    for (int k = 0; k < 5; ++k) q[k] = (const uint8_t*)dev[k];
    bool pass = false;
    const int32_t sq = queries_in_subgroup(ctx, "bzk_params_load_bellman_checked", q, true, L, report, &pass);
    if (sq == BZK_OK && pass) return BZK_OK;
    bzk_params_free(ctx, *out);
    *out = nullptr;
    if (sq != BZK_OK) return sq;
    ctx->last_error = failure_text(report);
    return BZK_E_ARG;
}

int32_t bzk_params_load_bellman(bzk_ctx* ctx, const uint8_t* bytes, uint64_t len, uint32_t n_in, uint32_t n_aux, const uint8_t* a_density,
                                const uint8_t* b_density, bzk_params** out, uint8_t* vk_out, uint64_t vk_cap) {
    return load_bellman(ctx, bytes, len, n_in, n_aux, a_density, b_density, out, vk_out, vk_cap, nullptr);
}
int32_t bzk_params_load_bellman_checked(bzk_ctx* ctx, const uint8_t* bytes, uint64_t len, uint32_t n_in, uint32_t n_aux, const uint8_t* a_density,
                                        const uint8_t* b_density, bzk_params** out, uint8_t* vk_out, uint64_t vk_cap, uint64_t report[4]) {
    if (!report) return BZK_E_ARG;
    return load_bellman(ctx, bytes, len, n_in, n_aux, a_density, b_density, out, vk_out, vk_cap, report);
}

// `Parameters::read(reader, checked = true)` as a verdict: 1, or 0 with report = {array, index, verdict code, 0} of the first failure in file order
int32_t bzk_bellman_params_check(bzk_ctx* ctx, const uint8_t* bytes, uint64_t len, uint64_t report[4]) {
    if (!bytes || !report) return BZK_E_ARG;
    report[0] = report[1] = report[2] = report[3] = 0;
    Decoded D;
    if (!decode_located(bytes, len, D, report) || !head_in_subgroup(D, report)) return 0;
    const uint8_t* q[5] = {D.h.data(), D.l.data(), D.a.data(), D.b1.data(), D.b2.data()};
    bool pass = false;
    const int32_t st = queries_in_subgroup(ctx, "bzk_bellman_params_check", q, false, D.L, report, &pass);
    if (st != BZK_OK) return st;
    return pass ? 1 : 0;
}

// The phase-2 step on a blob: h and l times d^-1 (bzk_g1_scale_batch's rounds: on the device with a context, on host threads without), the two deltas
// times d on the host, everything else as it was
int32_t bzk_bellman_params_rekey(bzk_ctx* ctx, const uint8_t* bytes, uint64_t len, const uint8_t d[32], uint8_t* out, uint64_t cap,
                                 uint64_t* size_out) {
    Layout L;
    if (!bytes || !d || !layout_of(bytes, len, L)) return BZK_E_ARG;
    uint8_t dinv[32];
    BZK_TRY(rekey_scalars(d, dinv));
    if (size_out) *size_out = L.total;
    if (!out) { wipe_host(dinv, sizeof dinv); return BZK_OK; }
    if (cap < L.total) { wipe_host(dinv, sizeof dinv); return BZK_E_ARG; }
    Decoded D;
    D.L = L;
    D.vk.resize(870); D.ic.resize(97 * L.n_ic); D.h.resize(96 * L.n_h); D.l.resize(96 * L.n_l); D.a.resize(96 * L.n_a);
    D.b1.resize(96 * L.n_b1); D.b2.resize(192 * L.n_b2);
    int32_t st = L.n_b1 != L.n_b2 ? BZK_E_ARG
                                  : bzk_bellman_params_decode(bytes, len, D.vk.data(), D.ic.data(), D.h.data(), D.l.data(), D.a.data(), D.b1.data(), D.b2.data(), 0);
    if (st == BZK_OK) st = g1_scale_run(ctx, "bzk_bellman_params_rekey", D.h.data(), false, L.n_h, dinv, D.h.data(), nullptr);
    if (st == BZK_OK) st = g1_scale_run(ctx, "bzk_bellman_params_rekey", D.l.data(), false, L.n_l, dinv, D.l.data(), nullptr);
    wipe_host(dinv, sizeof dinv);
    if (st != BZK_OK) return st;
    rekey_vk_head(D.vk.data(), d);
    return bzk_bellman_params_encode(D.vk.data(), D.ic.data(), L.n_ic, D.h.data(), L.n_h, D.l.data(), L.n_l, D.a.data(), L.n_a, D.b1.data(), D.b2.data(),
                                     L.n_b1, out, cap, nullptr);
}

// Is `after` a re-key of `before`?  The order of the tests is the order of bzk.h's description; report names the first that fails
int32_t bzk_bellman_params_rekey_check(bzk_ctx* ctx, const uint8_t* before, uint64_t before_len, const uint8_t* after, uint64_t after_len,
                                       const uint8_t seed[32], uint64_t report[4]) {
    if (!before || !after || !seed || !report) return BZK_E_ARG;
    report[0] = report[1] = report[2] = report[3] = 0;
    Decoded B, A;
    uint64_t where[4];  // a blob that does not decode is array 7 here, whichever record it was
    if (!decode_located(before, before_len, B, where) || !decode_located(after, after_len, A, where)) return fail_at(report, 7, 0, 2), 0;
    const Layout &LB = B.L, &LA = A.L;
    if (LB.n_ic != LA.n_ic || LB.n_h != LA.n_h || LB.n_l != LA.n_l || LB.n_a != LA.n_a || LB.n_b1 != LA.n_b1 || LB.n_b2 != LA.n_b2)
        return fail_at(report, 7, 0, 2), 0;
    // what a re-key leaves alone: alpha_g1, beta_g1, beta_g2, gamma_g2 (head points 0 .. 3), ic, a, b_g1, b_g2
    for (uint64_t k = 0; k < 4; ++k)
        if (memcmp(B.vk.data() + HEAD[k].dst, A.vk.data() + HEAD[k].dst, HEAD[k].g2 ? 193 : 97)) return fail_at(report, 0, k, 0), 0;
    struct Same { const std::vector<uint8_t>*b, *a; uint64_t sz, array; };
    const Same same[4] = {{&B.ic, &A.ic, 97, 1}, {&B.a, &A.a, 96, 4}, {&B.b1, &A.b1, 96, 5}, {&B.b2, &A.b2, 192, 6}};
    for (const Same& s : same)
        for (uint64_t i = 0; i * s.sz < s.b->size(); ++i)
            if (memcmp(s.b->data() + i * s.sz, s.a->data() + i * s.sz, s.sz)) return fail_at(report, s.array, i, 0), 0;
    // after's delta_g1, delta_g2, h, l in the order-r subgroup
    for (uint64_t k = 4; k < 6; ++k) {
        const uint8_t* p = A.vk.data() + HEAD[k].dst;
        if (p[HEAD[k].g2 ? 192 : 96]) return fail_at(report, 0, k, 2), 0;  // an identity delta is no key
        const uint8_t v = sg_host_one(HEAD[k].g2, p);
        if (v != 1) return fail_at(report, 0, k, v), 0;
    }
    const uint8_t* q[2] = {A.h.data(), A.l.data()};
    const uint64_t cnt[2] = {LA.n_h, LA.n_l};
    for (int k = 0; k < 2; ++k) {
        uint64_t idx = 0;
        uint8_t code = 1;
        BZK_TRY(sg_first_bad(ctx, "bzk_bellman_params_rekey_check", false, q[k], false, cnt[k], &idx, &code));
        if (idx < cnt[k]) return fail_at(report, 2 + k, idx, code), 0;
    }
    // delta the same multiple in both groups, before and after
    if (!rekey_delta_consistent(B.vk.data()) || !rekey_delta_consistent(A.vk.data())) return fail_at(report, 0, 5, 0), 0;
    // the ratio, over h and over l
    const uint8_t* qb[2] = {B.h.data(), B.l.data()};
    for (int k = 0; k < 2; ++k) {
        bool holds = false;
        BZK_TRY(rekey_ratio(ctx, (uint8_t)(2 + k), qb[k], q[k], cnt[k], seed, B.vk.data(), A.vk.data(), &holds));
        if (!holds) return fail_at(report, 2 + k, 0, 0), 0;
    }
    return 1;
}

}  // extern "C"
