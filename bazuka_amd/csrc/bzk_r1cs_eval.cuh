// A.z, B.z, C.z of an R1CS from the witness alone: the per-chunk and per-row functions the device kernels (r1cs_eval.hip), the host-thread route
// and the host check program (tests/host/r1cs_eval_check.hip) all run, and the host code that validates three CSR matrices and builds the
// resident form from them.
//
// Resident form of one matrix: row_ptr (u32, as given) | col (u32 per entry) | cidx (u32 per entry: index into the handle's dictionary of
// DISTINCT coefficients).  A dictionary entry is the coefficient c as  c * 2^261 mod r  in nine 29-bit limbs, canonical, padded to 12 words.
// A term is then ONE product without any conversion: the Montgomery-256 z entry (value z * 2^256) is repacked into 29-bit limbs as it is
// (repack_from32, no arithmetic), and  wide_reduce(sum (c 2^261) (z 2^256))  =  sum c z * 2^256  - the memory form of the result.
//
// Chunk bound (bzk_fr29.cuh): wide_mac adds 9 partial products of < 2^58 to a 64-bit column, wide_reduce another 9: at most SIX products
// per reduction (7 * 9 * 2^58 < 2^64), whatever the values.  The value bound needs sum ka * kb <= 70: a dictionary entry is < r (k 1), a
// repacked z entry is < 2^256 < 3 r even when its limbs are not a residue's (k 3): 6 * 3 = 18.  A row is therefore cut into chunks of at
// most 6 terms; every chunk's result is brought to [0, r) and the partial results are added modulo r - the running sum is always canonical,
// so a row may be as long as it likes and the last step is repack_to32 alone.
#pragma once
#include <stdint.h>

#include "bzk_field.cuh"
#include "bzk_fr29.cuh"

#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/bzk.h"

namespace bzk {
namespace r1e {

static constexpr uint32_t CHUNK = 6;        // products per reduction
static constexpr uint32_t DICT_WORDS = 12;  // words per dictionary entry: 9 limbs, padded to 48 B
static constexpr uint32_t SHORT_MAX = 12;   // rows of up to two chunks take a lane each, longer ones a wave each
static constexpr uint32_t WAVE = 64;

// one matrix as the evaluation reads it (device pointers in the device copy, host pointers on the host route)
struct Mat {
    const uint32_t* row_ptr;
    const uint32_t* col;
    const uint32_t* cidx;
    const uint32_t* dict;        // the handle's dictionary (the same for A, B and C)
    const uint32_t* short_rows;  // indices of the rows with <= SHORT_MAX entries, ascending
    const uint32_t* long_rows;   // the others, ascending
    uint32_t n_short, n_long;
    uint64_t n_rows;
};

// t - r where t >= r, t otherwise: [0, 2r) -> [0, r).  t normalised.
BZK_HD Fr29 cond_sub_r(const Fr29& t) {
    Fr29 s;
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < fr29::N; ++i) {
        const uint32_t d = t.l[i] - fr29::R.v[i] - borrow;
        borrow = d >> 31;
        s.l[i] = d & fr29::MASK;
    }
    return borrow ? t : s;
}
// a + b mod r for canonical a, b
BZK_HD Fr29 add_mod(const Fr29& a, const Fr29& b) { return cond_sub_r(fr29::norm(fr29::add(a, b))); }

// sum of the terms [b, e), e - b <= CHUNK, as a canonical residue (times 2^256)
BZK_HD Fr29 chunk_sum(const Mat& M, const Fr* z, uint32_t b, uint32_t e) {
    fr29::Wide w;
    fr29::wide_zero(w);
#pragma unroll 1
    for (uint32_t k = b; k < e; ++k) {
        const uint32_t* d = M.dict + (size_t)M.cidx[k] * DICT_WORDS;
        Fr29 c;
#pragma unroll
        for (int i = 0; i < fr29::N; ++i) c.l[i] = d[i];
        const Fr v = z[M.col[k]];
        fr29::wide_mac(w, c, fr29::repack_from32(v));
    }
    return cond_sub_r(fr29::wide_reduce(w));
}
// the chunks first, first + stride, ... of the terms [b, e): a whole row with (0, 1), one lane's share of a long row with (lane, WAVE)
BZK_HD Fr29 range_sum(const Mat& M, const Fr* z, uint32_t b, uint32_t e, uint32_t first, uint32_t stride) {
    Fr29 acc = fr29::zero();
#pragma unroll 1
    for (uint64_t s = (uint64_t)b + (uint64_t)first * CHUNK; s < e; s += (uint64_t)stride * CHUNK) {
        const uint32_t ce = e - (uint32_t)s < CHUNK ? e : (uint32_t)s + CHUNK;
        acc = add_mod(acc, chunk_sum(M, z, (uint32_t)s, ce));
    }
    return acc;
}
BZK_HD Fr row_eval(const Mat& M, const Fr* z, uint64_t row) {
    return fr29::repack_to32(range_sum(M, z, M.row_ptr[row], M.row_ptr[row + 1], 0, 1));
}
// a * b == c for canonical Montgomery-256 scalars
BZK_HD bool row_holds(const Fr& a, const Fr& b, const Fr& c) {
    const Fr p = fe_mul<FrParams>(a, b);
    uint32_t diff = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) diff |= p.l[i] ^ c.l[i];
    return diff == 0;
}

// ---- host: validation and the resident form ---------------------------------------------------------------------------------------------------
static inline bool limbs_below_r(const uint8_t* v) {
    uint32_t l[8];
    memcpy(l, v, 32);
    for (int i = 7; i >= 0; --i) {
        if (l[i] < FrParams::MOD[i]) return true;
        if (l[i] > FrParams::MOD[i]) return false;
    }
    return false;
}
// the refusals of bzk_r1cs_mats_load; `err` names the matrix and the row.  Reads row_ptr[0 .. n_rows], col[0 .. nnz), val[0 .. 32 nnz) and nothing else
static inline bool validate(const bzk_csr* const M[3], uint32_t n_in, uint32_t n_aux, std::string& err) {
    static const char* const name = "ABC";
    const std::string who = "r1cs_mats_load: ";
    if (n_in == 0) { err = who + "n_in = 0 (variable 0 is ONE)"; return false; }
    const uint64_t n_vars = (uint64_t)n_in + n_aux;
    for (int k = 0; k < 3; ++k) {
        if (!M[k]) { err = who + "matrix " + name[k] + " is NULL"; return false; }
        if (M[k]->n_rows != M[0]->n_rows) {
            err = who + "matrix " + name[k] + " has " + std::to_string(M[k]->n_rows) + " rows, matrix A " + std::to_string(M[0]->n_rows);
            return false;
        }
        if (M[k]->n_rows >= 0xffffffffull) { err = who + "matrix " + name[k] + ": more than 2^32 - 2 rows"; return false; }
    }
    for (int k = 0; k < 3; ++k) {
        const bzk_csr& m = *M[k];
        const std::string mat = who + "matrix " + name[k];
        if (!m.row_ptr) { err = mat + ": row_ptr is NULL"; return false; }  // (n_rows + 1 >= 1 words are always expected)
        if (m.row_ptr[0] != 0) { err = mat + " row 0: row_ptr[0] = " + std::to_string(m.row_ptr[0]) + ", not 0"; return false; }
        for (uint64_t i = 0; i < m.n_rows; ++i)
            if (m.row_ptr[i + 1] < m.row_ptr[i]) {
                err = mat + " row " + std::to_string(i) + ": row_ptr descends from " + std::to_string(m.row_ptr[i]) + " to " + std::to_string(m.row_ptr[i + 1]);
                return false;
            }
        const uint32_t nnz = m.row_ptr[m.n_rows];
        if (nnz && !m.col) { err = mat + ": col is NULL with " + std::to_string(nnz) + " entries"; return false; }
        if (nnz && !m.val) { err = mat + ": val is NULL with " + std::to_string(nnz) + " entries"; return false; }
        for (uint64_t i = 0; i < m.n_rows; ++i)
            for (uint32_t e = m.row_ptr[i]; e < m.row_ptr[i + 1]; ++e) {
                if (m.col[e] >= n_vars) {
                    err = mat + " row " + std::to_string(i) + ": column " + std::to_string(m.col[e]) + " >= " + std::to_string(n_vars) + " variables";
                    return false;
                }
                if (!limbs_below_r(m.val + (size_t)e * 32)) {
                    err = mat + " row " + std::to_string(i) + ": the coefficient of column " + std::to_string(m.col[e]) + " has limbs >= r";
                    return false;
                }
            }
    }
    return true;
}

struct HostMats {
    uint32_t n_in = 0, n_aux = 0;
    uint64_t n_rows = 0, n_dict = 0, n_pm1 = 0;  // n_pm1: entries whose coefficient is +1 or -1
    std::vector<uint32_t> row_ptr[3], col[3], cidx[3], short_rows[3], long_rows[3];
    std::vector<uint32_t> dict;  // n_dict x DICT_WORDS
    uint64_t nnz(int k) const { return col[k].size(); }
    // what the resident form holds, in bytes
    uint64_t bytes() const {
        uint64_t w = dict.size();
        for (int k = 0; k < 3; ++k) w += row_ptr[k].size() + col[k].size() + cidx[k].size() + short_rows[k].size() + long_rows[k].size();
        return 4 * w;
    }
    Mat view(int k) const {
        return Mat{row_ptr[k].data(), col[k].data(), cidx[k].data(), dict.data(), short_rows[k].data(), long_rows[k].data(),
                   (uint32_t)short_rows[k].size(), (uint32_t)long_rows[k].size(), n_rows};
    }
};
// c * 2^256 (canonical Montgomery-256 bytes) -> c * 2^261 in canonical 29-bit limbs
static inline Fr29 dict_entry(const uint8_t* val) {
    Fr v;
    memcpy(v.l, val, 32);
    return cond_sub_r(fr29::to29(v));
}
// the resident form of three VALIDATED matrices
static inline void build(const bzk_csr* const M[3], uint32_t n_in, uint32_t n_aux, HostMats& out) {
    struct Key {
        uint64_t w[4];
        bool operator==(const Key& o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
    };
    struct KeyHash {
        size_t operator()(const Key& k) const { return (size_t)((k.w[0] * 0x9e3779b97f4a7c15ull) ^ (k.w[1] * 0xc2b2ae3d27d4eb4full) ^ (k.w[2] << 7) ^ k.w[3]); }
    };
    out = HostMats();
    out.n_in = n_in;
    out.n_aux = n_aux;
    out.n_rows = M[0]->n_rows;
    std::unordered_map<Key, uint32_t, KeyHash> index;
    Key one, minus_one;
    {
        Fr o = Fr::one(), m = fe_sub<FrParams>(Fr::zero(), o);
        memcpy(one.w, o.l, 32);
        memcpy(minus_one.w, m.l, 32);
    }
    for (int k = 0; k < 3; ++k) {
        const bzk_csr& m = *M[k];
        const uint32_t nnz = m.row_ptr[m.n_rows];
        out.row_ptr[k].assign(m.row_ptr, m.row_ptr + m.n_rows + 1);
        if (nnz) out.col[k].assign(m.col, m.col + nnz);
        out.cidx[k].resize(nnz);
        Key last;
        uint32_t last_idx = 0;
        bool have_last = false;
        for (uint32_t e = 0; e < nnz; ++e) {
            Key key;
            memcpy(key.w, m.val + (size_t)e * 32, 32);
            if (key == one || key == minus_one) ++out.n_pm1;
            if (!(have_last && key == last)) {  // runs of one coefficient (a bit decomposition's powers aside) skip the table
                auto it = index.find(key);
                if (it == index.end()) {
                    it = index.emplace(key, (uint32_t)index.size()).first;
                    const Fr29 c = dict_entry(m.val + (size_t)e * 32);
                    for (int i = 0; i < fr29::N; ++i) out.dict.push_back(c.l[i]);
                    for (uint32_t i = fr29::N; i < DICT_WORDS; ++i) out.dict.push_back(0);
                }
                last = key;
                last_idx = it->second;
                have_last = true;
            }
            out.cidx[k][e] = last_idx;
        }
        for (uint64_t i = 0; i < m.n_rows; ++i)
            (m.row_ptr[i + 1] - m.row_ptr[i] <= SHORT_MAX ? out.short_rows[k] : out.long_rows[k]).push_back((uint32_t)i);
    }
    out.n_dict = index.size();
}

}  // namespace r1e
}  // namespace bzk
