// Stand-alone harness of the witness-only evaluation's host code (bazuka_amd/csrc/bzk_r1cs_eval.cuh): built with the address and
// undefined-behaviour sanitizers (host code only) and with BZK_FP28_CHECK, so the column assertions of wide_mac / wide_reduce are live; run by
// tests/test_r1cs_eval_cpu.py as a child process.
//
//   r1cs_eval_check table IN OUT   IN: u64 n_vars, n_rows, nnz | row_ptr (n_rows + 1) u32 | col (nnz) u32 | val (nnz x 32 B) | z (n_vars x 32 B).
//                                  Validates and builds the resident form (the matrix stands for A, B and C), evaluates every row three ways -
//                                  row_eval; the long-row schedule of the kernel (64 lanes' range_sum shares added pairwise in the order of the
//                                  wave reduction); chunk_sum / add_mod by hand - requires the three to agree and writes n_rows x 32 B to OUT.
//   r1cs_eval_check refusals       every malformed matrix of bzk_r1cs_mats_load's refusal list through validate(), the arrays in heap blocks of
//                                  exactly their size, so that a read past a count the loader should have refused first is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bazuka_amd/csrc/bzk_r1cs_eval.cuh"

using namespace bzk;

#define CHECK(cond, what)                                                       \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "r1cs_eval_check: %s: %s fails\n", what, #cond);    \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

// a matrix whose arrays are heap blocks of exactly their size (null where empty and `null_empty`)
struct Csr {
    bzk_csr m;
    uint32_t *rp = nullptr, *col = nullptr;
    uint8_t* val = nullptr;
    Csr(const std::vector<uint32_t>& row_ptr, const std::vector<uint32_t>& cols, const std::vector<uint8_t>& vals) {
        rp = (uint32_t*)malloc(row_ptr.size() * 4);
        memcpy(rp, row_ptr.data(), row_ptr.size() * 4);
        if (!cols.empty()) {
            col = (uint32_t*)malloc(cols.size() * 4);
            memcpy(col, cols.data(), cols.size() * 4);
        }
        if (!vals.empty()) {
            val = (uint8_t*)malloc(vals.size());
            memcpy(val, vals.data(), vals.size());
        }
        m.n_rows = row_ptr.size() - 1;
        m.row_ptr = rp;
        m.col = col;
        m.val = val;
    }
    ~Csr() {
        free(rp);
        free(col);
        free(val);
    }
    Csr(const Csr&) = delete;
};

static bool same(const Fr& a, const Fr& b) { return memcmp(a.l, b.l, 32) == 0; }

static int run_table(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    CHECK(f, "open");
    uint64_t hd[3];
    CHECK(fread(hd, 8, 3, f) == 3, "header");
    const uint64_t n_vars = hd[0], n_rows = hd[1], nnz = hd[2];
    std::vector<uint32_t> rp(n_rows + 1), col(nnz);
    std::vector<uint8_t> val(nnz * 32);
    CHECK(fread(rp.data(), 4, rp.size(), f) == rp.size(), "row_ptr");
    CHECK(nnz == 0 || fread(col.data(), 4, nnz, f) == nnz, "col");
    CHECK(nnz == 0 || fread(val.data(), 32, nnz, f) == nnz, "val");
    Fr* z = (Fr*)malloc(n_vars * 32);  // a block of exactly the witness: a column past it is a report
    CHECK(fread(z, 32, n_vars, f) == n_vars, "z");
    fclose(f);
    Csr A(rp, col, val);
    const bzk_csr* M[3] = {&A.m, &A.m, &A.m};
    std::string err;
    CHECK(r1e::validate(M, 1, (uint32_t)(n_vars - 1), err), err.c_str());
    r1e::HostMats H;
    r1e::build(M, 1, (uint32_t)(n_vars - 1), H);
    CHECK(H.short_rows[0].size() + H.long_rows[0].size() == n_rows, "row split");
    std::vector<Fr> out(n_rows);
    for (int k = 0; k < 3; ++k) {
        const r1e::Mat V = H.view(k);
        for (uint64_t i = 0; i < n_rows; ++i) {
            const uint32_t b = V.row_ptr[i], e = V.row_ptr[i + 1];
            const Fr direct = r1e::row_eval(V, z, i);
            // the wave schedule: lane l sums the chunks l, l + 64, ...; then lane l takes lane l + off for off = 32 .. 1
            Fr29 lane[r1e::WAVE];
            for (uint32_t l = 0; l < r1e::WAVE; ++l) lane[l] = r1e::range_sum(V, z, b, e, l, r1e::WAVE);
            for (uint32_t off = r1e::WAVE / 2; off >= 1; off >>= 1)
                for (uint32_t l = 0; l + off < r1e::WAVE; ++l) lane[l] = r1e::add_mod(lane[l], lane[l + off]);
            CHECK(same(direct, fr29::repack_to32(lane[0])), "wave schedule == one lane");
            // by hand, the chunks from the row's end: other cuts, the same residue
            Fr29 acc = fr29::zero();
            for (uint32_t hi = e; hi > b;) {
                const uint32_t lo = hi - b > r1e::CHUNK ? hi - r1e::CHUNK : b;
                acc = r1e::add_mod(acc, r1e::chunk_sum(V, z, lo, hi));
                hi = lo;
            }
            CHECK(same(direct, fr29::repack_to32(acc)), "chunks cut from the end == chunks cut from the start");
            if (k == 0) out[i] = direct;
            else CHECK(same(direct, out[i]), "the same matrix as B / C");
        }
    }
    free(z);
    f = fopen(out_path, "wb");
    CHECK(f, "open out");
    CHECK(n_rows == 0 || fwrite(out.data(), 32, n_rows, f) == n_rows, "write");
    fclose(f);
    printf("table holds: %llu rows, %llu entries, %llu coefficients, %zu long rows\n", (unsigned long long)n_rows, (unsigned long long)nnz,
           (unsigned long long)H.n_dict, H.long_rows[0].size());
    return 0;
}

static std::vector<uint8_t> mont_one(size_t n) {
    std::vector<uint8_t> v(n * 32);
    const Fr one = Fr::one();
    for (size_t i = 0; i < n; ++i) memcpy(v.data() + 32 * i, one.l, 32);
    return v;
}

static int n_refusals = 0;
static void refused(const char* what, const Csr& a, const Csr& b, const Csr& c, uint32_t n_in, uint32_t n_aux, const char* must_name, const char* row) {
    const bzk_csr* M[3] = {&a.m, &b.m, &c.m};
    std::string err;
    CHECK(!r1e::validate(M, n_in, n_aux, err), what);
    if (must_name && err.find(must_name) == std::string::npos) {
        fprintf(stderr, "r1cs_eval_check: %s: '%s' does not name '%s'\n", what, err.c_str(), must_name);
        exit(1);
    }
    if (row && err.find(row) == std::string::npos) {
        fprintf(stderr, "r1cs_eval_check: %s: '%s' does not name '%s'\n", what, err.c_str(), row);
        exit(1);
    }
    ++n_refusals;
}

static int run_refusals() {
    // the good triple: 3 rows over 4 variables
    const std::vector<uint32_t> rp = {0, 2, 2, 3}, col = {0, 3, 1};
    const std::vector<uint8_t> val = mont_one(3);
    Csr good(rp, col, val);
    {
        const bzk_csr* M[3] = {&good.m, &good.m, &good.m};
        std::string err;
        CHECK(r1e::validate(M, 2, 2, err), "the good triple");
    }
    {   // the three n_rows differ
        Csr two({0, 2, 3}, col, val);
        refused("n_rows differ (B)", good, two, good, 2, 2, "matrix B", nullptr);
        refused("n_rows differ (C)", good, good, two, 2, 2, "matrix C", nullptr);
    }
    {   // row_ptr[0] != 0: the counts then run past the arrays - nothing behind row_ptr may be read
        Csr bad({1, 2, 2, 3}, col, val);
        refused("row_ptr[0] != 0", bad, good, good, 2, 2, "matrix A", "row 0");
        refused("row_ptr[0] != 0 (C)", good, good, bad, 2, 2, "matrix C", "row 0");
    }
    {   // row_ptr descends (its last word is smaller than an earlier one, and an earlier one is past the arrays)
        Csr bad({0, 9, 2, 3}, col, val);
        refused("row_ptr descends", good, bad, good, 2, 2, "matrix B", "row 1");
        Csr last({0, 2, 3, 1}, col, val);
        refused("row_ptr descends at its end", last, good, good, 2, 2, "matrix A", "row 2");
    }
    {   // a column >= n_in + n_aux
        Csr bad(rp, {0, 3, 4}, val);
        refused("column out of range", good, good, bad, 2, 2, "matrix C", "row 2");
        refused("column out of range for a smaller shape", good, good, good, 2, 1, "matrix A", "row 0");
        Csr huge(rp, {0, 0xffffffffu, 1}, val);
        refused("column 2^32 - 1", huge, good, good, 2, 2, "matrix A", "row 0");
    }
    {   // a coefficient whose limbs are >= r: r itself, 2^256 - 1
        std::vector<uint8_t> v = val;
        memcpy(v.data() + 64, FrParams::MOD, 32);
        Csr bad(rp, col, v);
        refused("coefficient = r", good, bad, good, 2, 2, "matrix B", "row 2");
        memset(v.data() + 64, 0, 32);
        memset(v.data(), 0xff, 32);
        Csr bad2(rp, col, v);
        refused("coefficient = 2^256 - 1", bad2, good, good, 2, 2, "matrix A", "row 0");
        uint32_t below[8];  // r - 1 loads
        memcpy(below, FrParams::MOD, 32);
        below[0] -= 1;
        memcpy(v.data(), below, 32);
        Csr ok(rp, col, v);
        const bzk_csr* M[3] = {&ok.m, &good.m, &good.m};
        std::string err;
        CHECK(r1e::validate(M, 2, 2, err), "coefficient r - 1 loads");
    }
    {   // a NULL array with a non-zero count
        Csr nocol(rp, {}, val), noval(rp, col, {});
        refused("col NULL", nocol, good, good, 2, 2, "matrix A", "col");
        refused("val NULL", good, noval, good, 2, 2, "matrix B", "val");
        Csr norp(rp, col, val);
        norp.m.row_ptr = nullptr;
        refused("row_ptr NULL", good, good, norp, 2, 2, "matrix C", "row_ptr");
        const bzk_csr* M[3] = {&good.m, nullptr, &good.m};
        std::string err;
        CHECK(!r1e::validate(M, 2, 2, err) && err.find("matrix B") != std::string::npos, "a NULL matrix");
        ++n_refusals;
        // ... while NULL col / val with NO entries load: three empty rows
        Csr empty({0, 0, 0, 0}, {}, {});
        const bzk_csr* E[3] = {&empty.m, &empty.m, &empty.m};
        CHECK(r1e::validate(E, 2, 2, err), "empty rows, NULL col and val");
        r1e::HostMats H;
        r1e::build(E, 2, 2, H);
        const Fr z[4] = {Fr::one(), Fr::one(), Fr::one(), Fr::one()};
        CHECK(r1e::row_eval(H.view(1), z, 2).is_zero(), "an empty row evaluates to zero");
    }
    refused("n_in = 0", good, good, good, 0, 4, "n_in", nullptr);
    printf("%d refusals hold\n", n_refusals);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "table")) return run_table(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "refusals")) return run_refusals();
    fprintf(stderr, "usage: r1cs_eval_check table IN OUT | refusals\n");
    return 2;
}
