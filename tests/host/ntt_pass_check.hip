// CPU replay of the NTT passes (bazuka_amd/csrc/ntt.hip: ntt_pass_kernel, ntt_tables, ntt_run_ex, ntt_h_chain) with the bound arguments of its comments
// asserted on exact integers.  A stand-alone program, built with BZK_FP28_CHECK (the column assertions of bzk_fr29.cuh) and the address and
// undefined-behaviour sanitizers (host code only):
//     _ntt_pass_check ntt <log_n> <bmax> <in> <out>    in: k vectors of n raw 32-byte elements; out: per vector the four transforms (inverse, coset) =
//                                                      (0,0) (0,1) (1,0) (1,1), n elements each
//     _ntt_pass_check h <log_m> <bmax> <in> <out>      in: k triples a | b | c of m elements each (padded); out: per triple the m elements a holds after
//                                                      the fused chain 3 x (NTT_INV_TO_COSET, NTT_FWD_RAW / NTT_FWD_RAW_S5), NTT_INV_COSET_PW
// Whole transforms run through the plan's passes on host arrays: plain loops for the indexing (one column at a time - the tile width CC only groups
// independent columns), twiddle and scaling tables built with the host field (fe_mul<FrParams>), 32-byte inter-pass elements.  The ARITHMETIC below
// marked "restated" is ntt.hip's, line for line (moving it into a header both would share changed the kernels' register counts and code, so the kernel
// keeps its text; the comments there name this file): change one and change the other.
// Asserted, all on the limbs as integers:
//   - ka * kb <= 70 at every product (A * B <= 70 r^2)
//   - at every sub3 each subtrahend limb is at most the D3 limb and no 32-bit word wraps (additions and carries included)
//   - every value given to repack_to32 is normalised and below 2^256
//   - k <= 35 (A <= 35 r) and s < r at from29_scaled
// A violated bound prints the site and aborts.  On success one line: the largest ka * kb at a product and the largest k at a store that were seen.
#define BZK_FP28_CHECK 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include "../../bazuka_amd/csrc/bzk_field.cuh"
#include "../../bazuka_amd/csrc/bzk_fr29.cuh"

using namespace bzk;

// ---------------------------------------------------------------------------------------------------------------- exact integers
typedef unsigned __int128 u128;
struct Big {
    uint64_t w[10];
};
static Big big_from_limbs(const uint32_t* l) {  // sum l[i] 2^(29 i), any 32-bit limbs: below 2^264
    Big r;
    memset(&r, 0, sizeof r);
    for (int i = 0; i < 9; ++i) {
        const int bit = 29 * i, k = bit >> 6, sh = bit & 63;
        u128 v = (u128)l[i] << sh;
        for (int j = k; v; ++j) {
            v += r.w[j];
            r.w[j] = (uint64_t)v;
            v >>= 64;
        }
    }
    return r;
}
static Big big_mul5(const Big& a, const Big& b) {  // operands below 2^320
    Big r;
    memset(&r, 0, sizeof r);
    for (int i = 0; i < 5; ++i) {
        uint64_t c = 0;
        for (int j = 0; j < 5; ++j) {
            const u128 t = (u128)a.w[i] * b.w[j] + r.w[i + j] + c;
            r.w[i + j] = (uint64_t)t;
            c = (uint64_t)(t >> 64);
        }
        r.w[i + 5] = c;
    }
    return r;
}
static Big big_small(const Big& a, uint64_t m) {
    Big r;
    uint64_t c = 0;
    for (int i = 0; i < 10; ++i) {
        const u128 t = (u128)a.w[i] * m + c;
        r.w[i] = (uint64_t)t;
        c = (uint64_t)(t >> 64);
    }
    if (c) abort();
    return r;
}
static int big_cmp(const Big& a, const Big& b) {
    for (int i = 9; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
static double big_double(const Big& a) {
    double v = 0;
    for (int i = 9; i >= 0; --i) v = v * 18446744073709551616.0 + (double)a.w[i];
    return v;
}

static Big B_R, B_35R, B_70R2;
static uint64_t QUICK_T;  // floor(70 r^2 / 2^464)
static double D_R;

struct Stats {
    double max_kakb = 0, max_k_final = 0, max_k_col = 0;
    uint64_t products = 0, exact = 0;
};
static thread_local Stats* g_st = nullptr;

[[noreturn]] static void violated(const char* what, const Fr29& a, const Fr29* b) {
    fprintf(stderr, "BOUND VIOLATED: %s\n  a =", what);
    for (int i = 0; i < 9; ++i) fprintf(stderr, " %08x", a.l[i]);
    if (b) {
        fprintf(stderr, "\n  b =");
        for (int i = 0; i < 9; ++i) fprintf(stderr, " %08x", b->l[i]);
    }
    fprintf(stderr, "\n");
    abort();
}

// value / r in floating point: only for the figures that are REPORTED, never for an assertion
static double k_of(const Fr29& a) {
    double v = 0;
    for (int i = 8; i >= 0; --i) v = v * 536870912.0 + (double)a.l[i];
    return v / D_R;
}

// ka * kb <= 70, exactly: A * B <= 70 r^2.  With every limb a 32-bit word A < (l[8] + 9) 2^232, so (la + 9)(lb + 9) <= floor(70 r^2 / 2^464) already
// proves it in two integer operations; only operands near the limit take the 10-word product.
static void check_product(const Fr29& a, const Fr29& b, const char* site) {
    Stats& st = *g_st;
    ++st.products;
    const u128 q = (u128)((uint64_t)a.l[8] + 9) * ((uint64_t)b.l[8] + 9);
    if (q > QUICK_T) {
        ++st.exact;
        if (big_cmp(big_mul5(big_from_limbs(a.l), big_from_limbs(b.l)), B_70R2) > 0) violated(site, a, &b);
    }
    const double kk = k_of(a) * k_of(b);
    if (kk > st.max_kakb) st.max_kakb = kk;
}
static void check_add(const Fr29& a, const Fr29& b) {  // norm(add(a, b)): no word wraps
    uint64_t c = 0;
    for (int i = 0; i < 9; ++i) {
        const uint64_t t = (uint64_t)a.l[i] + b.l[i] + c;
        if (t >> 32) violated("add + norm: a 32-bit word wraps", a, &b);
        c = t >> 29;
    }
}
static void check_sub3(const Fr29& a, const Fr29& b) {
    uint64_t c = 0;
    for (int i = 0; i < 9; ++i) {
        if (b.l[i] > fr29::D3.v[i]) violated("sub3: a subtrahend limb exceeds its D3 limb", a, &b);
        const uint64_t t = (uint64_t)a.l[i] + fr29::D3.v[i] - b.l[i] + c;
        if (t >> 32) violated("sub3: a 32-bit word wraps", a, &b);
        c = t >> 29;
    }
}
static void check_repack(const Fr29& a) {  // repack_to32: normalised and below 2^256 = 2^(232 + 24)
    for (int i = 0; i < 8; ++i)
        if (a.l[i] > fr29::MASK) violated("repack_to32: not normalised", a, nullptr);
    if (a.l[8] >> 24) violated("repack_to32: value not below 2^256", a, nullptr);
}

static Fr29 cmul(const Fr29& a, const Fr29& b, const char* site) {
    check_product(a, b, site);
    return fr29::mul(a, b);  // on the host mul == mul_body
}
static Fr29 cadd(const Fr29& a, const Fr29& b) {
    check_add(a, b);
    return fr29::norm(fr29::add(a, b));
}
static Fr29 csub3(const Fr29& a, const Fr29& b) {
    check_sub3(a, b);
    return fr29::sub3(a, b);
}

// ---------------------------------------------------------------------------------------------------------------- restated from ntt.hip
enum { FIRST_MUL = 0, FIRST_RAW = 1, FIRST_PW = 2 };
enum { NTT_PLAIN = 0, NTT_INV_TO_COSET = 1, NTT_FWD_RAW = 2, NTT_FWD_RAW_S5 = 3, NTT_INV_COSET_PW = 4 };

// restated: ntt_first_load
static Fr29 first_load(int first_mode, const Fr& xr, const Fr* yr, const Fr* zr, const Fr29& kmul, const Fr29* pre, const Fr29& c_in) {
    const Fr29 x = fr29::repack_from32(xr);
    if (first_mode == FIRST_RAW) return x;
    if (first_mode == FIRST_PW) {
        const Fr29 y = fr29::repack_from32(*yr);
        const Fr29 z = fr29::repack_from32(*zr);
        return cmul(csub3(cmul(x, y, "FIRST_PW a * b"), z), kmul, "FIRST_PW (a b - c) * kmul");
    }
    return cmul(x, pre ? *pre : c_in, "FIRST_MUL");
}
// restated: the lone stage of ntt_pass_kernel (an odd stage count starts with it)
static void lone_stage(Fr29& e0, Fr29& e1) {
    const Fr29 u = e0, t = e1;
    e0 = cadd(u, t);
    e1 = csub3(u, t);
}
// restated: one radix-4 round of ntt_pass_kernel (stages s and s + 1 in registers)
static void round4(Fr29& e0, Fr29& e1, Fr29& e2, Fr29& e3, const Fr29& wa, const Fr29& wb, const Fr29& wc, int s) {
    Fr29 x0 = e0, x1 = e1, x2 = e2, x3 = e3;
    if (s) {
        x1 = cmul(x1, wa, "stage s: x1 * wa");
        x3 = cmul(x3, wa, "stage s: x3 * wa");
    }
    const Fr29 y0 = cadd(x0, x1), y1 = csub3(x0, x1);
    const Fr29 y2 = cadd(x2, x3), y3 = csub3(x2, x3);
    const Fr29 u2 = cmul(y2, wb, "stage s + 1: y2 * wb");
    const Fr29 u3 = cmul(y3, wc, "stage s + 1: y3 * wc");
    e0 = cadd(y0, u2);
    e2 = csub3(y0, u2);
    e1 = cadd(y1, u3);
    e3 = csub3(y1, u3);
}
// restated: the digit split of ntt_tables; returns nb, 0 where the first digit would exceed 10 bits
static int digit_split(int log_n, int bm, int b[3]) {
    b[0] = b[1] = b[2] = 0;
    if (log_n <= bm) { b[0] = log_n; return 1; }
    if (log_n <= 2 * bm) { b[0] = (log_n + 1) / 2; b[1] = log_n / 2; return 2; }
    b[0] = (log_n + 2) / 3;
    const int rest = log_n - b[0];
    b[1] = (rest + 1) / 2;
    b[2] = rest / 2;
    return b[0] > 10 ? 0 : 3;
}
// restated: from29_scaled's caller contract (any ka <= 35, s < r), then the function itself
static Fr final_store(const Fr29& v, const Fr29& s) {
    if (big_cmp(big_from_limbs(v.l), B_35R) > 0) violated("from29_scaled: k > 35", v, &s);
    if (big_cmp(big_from_limbs(s.l), B_R) >= 0) violated("from29_scaled: s >= r", v, &s);
    check_product(v, s, "from29_scaled");
    // what from29_scaled gives to repack_to32 is t = v s 2^-261 or t - r: t itself is checked (normalised, below 2^256), which covers both
    check_repack(fr29::mul(v, s));
    const double k = k_of(v);
    if (k > g_st->max_k_final) g_st->max_k_final = k;
    return fr29::from29_scaled(v, s);
}

// ---------------------------------------------------------------------------------------------------------------- host field, tables
static Fr h_pow(Fr b, uint64_t e) {
    Fr r = Fr::one();
    while (e) {
        if (e & 1) r = fe_mul<FrParams>(r, b);
        b = fe_sqr<FrParams>(b);
        e >>= 1;
    }
    return r;
}
static Fr h_u64(uint64_t v) {
    Fr c = Fr::zero();
    c.l[0] = (uint32_t)v;
    c.l[1] = (uint32_t)(v >> 32);
    return fe_to_mont<FrParams>(c);
}
static Fr h_omega(int log_n) {  // (7^((r - 1) / 2^32))^(2^(32 - log_n))
    uint32_t e[8];
    uint64_t borrow = 1;
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)FrParams::MOD[i] - borrow;
        e[i] = (uint32_t)d;
        borrow = (d >> 63) & 1;
    }
    const Fr g = h_u64(7);
    Fr w = Fr::one();
    for (int i = 255; i >= 32; --i) {
        w = fe_sqr<FrParams>(w);
        if ((e[i >> 5] >> (i & 31)) & 1) w = fe_mul<FrParams>(w, g);
    }
    for (int i = log_n; i < 32; ++i) w = fe_sqr<FrParams>(w);
    return w;
}
// out[j] = the nine 29-bit limbs of the raw Montgomery-256 value of base^j * c (ntt_table29_kernel)
static std::vector<Fr29> table29(const Fr& base, uint64_t count, const Fr& c) {
    std::vector<Fr29> t(count ? count : 1);
    Fr p = Fr::one();
    for (uint64_t j = 0; j < t.size(); ++j) {
        t[j] = fr29::repack_from32(fe_mul<FrParams>(p, c));
        p = fe_mul<FrParams>(p, base);
    }
    return t;
}

struct Tables {
    int log_n = 0, nb = 0, b[3] = {0, 0, 0};
    uint64_t n = 0;
    std::vector<Fr29> tw_r[2][3], tlo[2][2], thi[2][2], tone[2][2];
    std::vector<Fr29> pre_g, post_ginv, post_g, post_one;  // post_one[4] = kmul
};
static void build_tables(Tables& T, int log_n, int bmax) {
    T.log_n = log_n;
    T.n = (uint64_t)1 << log_n;
    T.nb = digit_split(log_n, bmax, T.b);
    if (!T.nb) {
        fprintf(stderr, "no plan for log_n %d with bmax %d\n", log_n, bmax);
        exit(2);
    }
    const uint64_t n = T.n;
    const Fr w = h_omega(log_n), g = h_u64(7);
    const Fr dirs[2] = {w, fe_inv<FrParams>(w)};
    const Fr c5 = h_u64(32), c0 = Fr::one();
    for (int d = 0; d < 2; ++d) {
        for (int k = 0; k < T.nb; ++k) {
            const uint64_t R = (uint64_t)1 << T.b[k];
            T.tw_r[d][k] = table29(h_pow(dirs[d], n / R), R / 2 ? R / 2 : 1, c5);
        }
        for (int k = 0; k + 1 < T.nb; ++k) {
            const uint64_t np = k == 0 ? n : n >> T.b[0];
            const Fr base = k == 0 ? dirs[d] : h_pow(dirs[d], (uint64_t)1 << T.b[0]);
            T.tlo[d][k] = table29(base, 1024, c5);
            T.thi[d][k] = table29(h_pow(base, 1024), (np + 1023) / 1024, c5);
            if (k > 0 && np <= ((uint64_t)1 << 17)) T.tone[d][k] = table29(base, np, c5);
        }
    }
    const Fr ninv = fe_inv<FrParams>(h_u64(n));
    const Fr zinv = fe_inv<FrParams>(fe_sub<FrParams>(h_pow(g, n), Fr::one()));
    const Fr five[5] = {Fr::one(), ninv, c5, fe_mul<FrParams>(ninv, c5), fe_mul<FrParams>(zinv, h_u64(32768))};
    for (int i = 0; i < 5; ++i) T.post_one.push_back(fr29::repack_from32(fe_mul<FrParams>(five[i], c0)));
    T.pre_g = table29(g, n, h_u64(1024));                                 // g^j 2^266
    T.post_ginv = table29(fe_inv<FrParams>(g), n, ninv);                 // g^-j / n 2^256
    T.post_g = table29(g, n, fe_mul<FrParams>(ninv, h_u64(32)));          // g^j / n 2^261
}

static uint32_t bitrev(uint32_t v, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// the R-point DFT of one column, already loaded bit-reversed: the stages of ntt_pass_kernel with CC = 1
static void column_dft(std::vector<Fr29>& col, int b, const std::vector<Fr29>& tw_r) {
    const uint32_t R = 1u << b;
    int s0 = 0;
    if (b & 1) {
        for (uint32_t bq = 0; bq < R / 2; ++bq) lone_stage(col[2 * bq], col[2 * bq + 1]);
        s0 = 1;
    }
    for (int s = s0; s < b; s += 2) {
        const uint32_t m = 1u << s;
        for (uint32_t bq = 0; bq < R / 4; ++bq) {
            const uint32_t j = bq & (m - 1);
            const uint32_t k0 = ((bq >> s) << (s + 2)) + j;
            const Fr29& wa = tw_r.at((size_t)j << (b - 1 - s));
            const Fr29& wb = tw_r.at((size_t)j << (b - 2 - s));
            const Fr29& wc = tw_r.at((size_t)(j + m) << (b - 2 - s));
            round4(col.at(k0), col.at(k0 + m), col.at(k0 + 2 * m), col.at(k0 + 3 * m), wa, wb, wc, s);
        }
    }
}

// ntt_run_ex: data is transformed in place; src_b / src_c only for NTT_INV_COSET_PW
static void run_ex(const Tables& T, std::vector<Fr>& data, int inverse, int coset, int fuse, const std::vector<Fr>* src_b, const std::vector<Fr>* src_c) {
    const uint64_t n = T.n;
    int first_mode = FIRST_RAW;
    const std::vector<Fr29>*pre = nullptr, *post = nullptr;
    const Fr29* post_c = nullptr;
    switch (fuse) {
        case NTT_INV_TO_COSET: inverse = 1; post = &T.post_g; break;
        case NTT_FWD_RAW: inverse = 0; post_c = &T.post_one[2]; break;
        case NTT_FWD_RAW_S5: inverse = 0; post_c = &T.post_one[0]; break;
        case NTT_INV_COSET_PW: inverse = 1; first_mode = FIRST_PW; post = &T.post_ginv; break;
        default:
            if (coset && !inverse) {
                first_mode = FIRST_MUL;
                pre = &T.pre_g;
                post_c = &T.post_one[0];
            } else if (coset) {
                first_mode = FIRST_MUL;
                post = &T.post_ginv;
            } else {
                post_c = &T.post_one[inverse ? 3 : 2];
            }
    }
    const int d = inverse ? 1 : 0;
    const Fr29 c_in = fr29::from_consts(fr29::C_IN);
    std::vector<Fr> tmp(T.nb > 1 ? n : 0);
    std::vector<Fr29> col;
    uint64_t S = n;
    for (int k = 0; k < T.nb; ++k) {
        const int b = T.b[k];
        const uint64_t R = (uint64_t)1 << b;
        S >>= b;
        const bool first_pass = k == 0, final_pass = k == T.nb - 1;
        const std::vector<Fr>& src = k == 0 ? data : tmp;
        col.assign(R, fr29::zero());
        auto load = [&](uint64_t addr) {
            if (!first_pass) return fr29::repack_from32(src.at(addr));
            return first_load(first_mode, src.at(addr), src_b ? &src_b->at(addr) : nullptr, src_c ? &src_c->at(addr) : nullptr, T.post_one[4],
                              pre ? &pre->at(addr) : nullptr, c_in);
        };
        if (!final_pass) {
            // COL pass: element (a, c) lives at src[base + a S + c]; row ka is multiplied by w_N'^(inner ka) and written to the same place of tmp.
            // A first pass reads data and writes tmp; the second of three reads and writes tmp, every column its own places
            const std::vector<Fr29>&tlo = T.tlo[d][k], &thi = T.thi[d][k], &tone = T.tone[d][k];
            for (uint64_t o = 0; o < n / (R * S); ++o) {
                for (uint64_t inner = 0; inner < S; ++inner) {
                    const uint64_t base = o * R * S + inner;
                    for (uint32_t r = 0; r < R; ++r) col[bitrev(r, b)] = load(base + (uint64_t)r * S);
                    column_dft(col, b, T.tw_r[d][k]);
                    for (uint32_t ka = 0; ka < R; ++ka) {
                        const uint64_t e = inner * ka;
                        Fr29 w;
                        if (!tone.empty()) {
                            w = tone.at(e);
                        } else {
                            w = tlo.at(e & 1023);
                            if (e >> 10) w = cmul(w, thi.at(e >> 10), "inter-pass twiddle lo * hi");
                        }
                        const double kk = k_of(col[ka]);
                        if (kk > g_st->max_k_col) g_st->max_k_col = kk;
                        const Fr29 ov = cmul(col[ka], w, "inter-pass store v * w");
                        check_repack(ov);
                        tmp.at(base + (uint64_t)ka * S) = fr29::repack_to32(ov);
                    }
                }
            }
        } else {
            const uint32_t R1 = T.nb >= 2 ? 1u << T.b[0] : 1u, R2 = T.nb == 3 ? 1u << T.b[1] : 1u;
            std::vector<Fr> out(n);
            for (uint32_t k2 = 0; k2 < R2; ++k2) {
                for (uint32_t k1 = 0; k1 < R1; ++k1) {
                    for (uint32_t r = 0; r < R; ++r) col[bitrev(r, b)] = load(((uint64_t)k1 * R2 + k2) * R + r);
                    column_dft(col, b, T.tw_r[d][k]);
                    for (uint32_t ka = 0; ka < R; ++ka) {
                        const uint64_t ko = (uint64_t)k1 + (uint64_t)R1 * (k2 + (uint64_t)R2 * ka);
                        out.at(ko) = final_store(col[ka], post ? post->at(ko) : *post_c);
                    }
                }
            }
            data.swap(out);
        }
    }
}

// ntt_h_chain
static void h_chain(const Tables& T, std::vector<Fr>& a, std::vector<Fr>& b, std::vector<Fr>& c) {
    std::vector<Fr>* v[3] = {&a, &b, &c};
    for (int k = 0; k < 3; ++k) {
        run_ex(T, *v[k], 1, 0, NTT_INV_TO_COSET, nullptr, nullptr);
        run_ex(T, *v[k], 0, 1, k == 2 ? NTT_FWD_RAW_S5 : NTT_FWD_RAW, nullptr, nullptr);
    }
    run_ex(T, a, 1, 1, NTT_INV_COSET_PW, &b, &c);
}

// ---------------------------------------------------------------------------------------------------------------- driver
static std::vector<Fr> to_fr(const uint8_t* p, uint64_t n) {
    std::vector<Fr> v(n);
    for (uint64_t i = 0; i < n; ++i) memcpy(v[i].l, p + 32 * i, 32);
    return v;
}

int main(int argc, char** argv) {
    if (argc != 6 || (strcmp(argv[1], "ntt") && strcmp(argv[1], "h"))) {
        fprintf(stderr, "usage: %s ntt|h <log_n> <bmax> <in> <out>\n", argv[0]);
        return 2;
    }
    const bool h = !strcmp(argv[1], "h");
    const int log_n = atoi(argv[2]), bmax = atoi(argv[3]);
    if (log_n < 1 || log_n > 24 || bmax < 4 || bmax > 10) {
        fprintf(stderr, "log_n 1 .. 24, bmax 4 .. 10\n");
        return 2;
    }
    const uint64_t n = (uint64_t)1 << log_n;
    FILE* f = fopen(argv[4], "rb");
    if (!f) {
        perror(argv[4]);
        return 2;
    }
    std::vector<uint8_t> in;
    {
        std::vector<uint8_t> buf(1 << 20);
        for (size_t k; (k = fread(buf.data(), 1, buf.size(), f)) > 0;) in.insert(in.end(), buf.begin(), buf.begin() + k);
    }
    fclose(f);
    const uint64_t rec = 32 * n * (h ? 3 : 1);
    if (in.empty() || in.size() % rec) {
        fprintf(stderr, "%zu bytes are not a whole number of %llu-byte records\n", in.size(), (unsigned long long)rec);
        return 2;
    }
    const uint64_t nrec = in.size() / rec;

    B_R = big_from_limbs(fr29::R.v);
    B_35R = big_small(B_R, 35);
    B_70R2 = big_small(big_mul5(B_R, B_R), 70);
    QUICK_T = (B_70R2.w[7] >> 16) | (B_70R2.w[8] << 48);  // >> 464
    if (B_70R2.w[9] || (B_70R2.w[8] >> 16)) abort();
    D_R = big_double(B_R);

    Tables T;
    build_tables(T, log_n, bmax);

    const uint64_t per = h ? 1 : 4, jobs = nrec * per;
    std::vector<uint8_t> out(32 * n * jobs);
    std::atomic<uint64_t> next(0);
    std::mutex mu;
    Stats total;
    auto worker = [&] {
        Stats st;
        g_st = &st;
        for (uint64_t j; (j = next.fetch_add(1)) < jobs;) {
            const uint8_t* p = in.data() + rec * (j / per);
            std::vector<Fr> a = to_fr(p, n);
            if (h) {
                std::vector<Fr> b = to_fr(p + 32 * n, n), c = to_fr(p + 64 * n, n);
                h_chain(T, a, b, c);
            } else {
                run_ex(T, a, (int)((j % 4) >> 1), (int)(j & 1), NTT_PLAIN, nullptr, nullptr);
            }
            for (uint64_t i = 0; i < n; ++i) memcpy(out.data() + 32 * (n * j + i), a[i].l, 32);
        }
        std::lock_guard<std::mutex> lk(mu);
        if (st.max_kakb > total.max_kakb) total.max_kakb = st.max_kakb;
        if (st.max_k_final > total.max_k_final) total.max_k_final = st.max_k_final;
        if (st.max_k_col > total.max_k_col) total.max_k_col = st.max_k_col;
        total.products += st.products;
        total.exact += st.exact;
    };
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
    if (nt > jobs) nt = (unsigned)jobs;
    std::vector<std::thread> th;
    for (unsigned i = 1; i < nt; ++i) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();

    f = fopen(argv[5], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f)) {
        perror(argv[5]);
        return 2;
    }
    printf("plan %d+%d+%d transforms %llu products %llu exact_checks %llu max_kakb %.2f max_k_final_store %.2f max_k_col_store %.2f\n", T.b[0], T.b[1], T.b[2],
           (unsigned long long)jobs, (unsigned long long)total.products, (unsigned long long)total.exact, total.max_kakb, total.max_k_final, total.max_k_col);
    return 0;
}
