// The per-point multiplication (bazuka_amd/csrc/bzk_pmul.cuh: row_of, power_of, mul_point over PmG1 / PmG2) in its DEVICE-field instantiation
// (sc::ScFp28: the 14 x 28-bit field, every product inlined, Fermat's inversion), run on the CPU with the bound assertions of bzk_fp28.cuh on.
// A stand-alone program, built with the address and undefined-behaviour sanitizers (host code only):
//     _pmul_check <g1|g2> <records file> scalars <file: 32 bytes per record, Montgomery Fr>
//     _pmul_check <g1|g2> <records file> powers <c: 64 hex digits> <s: 64 hex digits> <start>
// reads n raw records (96 or 192 bytes) and prints "inf <n digits>" and "out <hex>"; tests/test_point_mul_cpu.py compares them with the oracle's
// products.  An assertion (an operand outside the bounds the field documents) aborts.
#define BZK_FP28_CHECK 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../bazuka_amd/csrc/bzk_pmul.cuh"

using namespace bzk;

static bool read_file(const char* path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}
static bool hex32(const char* s, Fr& k) {
    if (strlen(s) != 64) return false;
    uint8_t b[32];
    for (int i = 0; i < 32; ++i) {
        unsigned v = 0;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        b[i] = (uint8_t)v;
    }
    memcpy(k.l, b, 32);
    return true;
}

int main(int argc, char** argv) {
    const bool scalars = argc == 5 && !strcmp(argv[3], "scalars"), powers = argc == 7 && !strcmp(argv[3], "powers");
    if (!(scalars || powers) || (strcmp(argv[1], "g1") && strcmp(argv[1], "g2"))) {
        fprintf(stderr, "usage: %s <g1|g2> <records file> scalars <file> | powers <c> <s> <start>\n", argv[0]);
        return 2;
    }
    const bool g2 = !strcmp(argv[1], "g2");
    const size_t sz = g2 ? 192 : 96;
    std::vector<uint8_t> recs, scal;
    if (!read_file(argv[2], recs) || recs.size() % sz) return 2;
    const size_t n = recs.size() / sz;
    Fr tab[65];
    uint64_t start = 0;
    if (scalars) {
        if (!read_file(argv[4], scal) || scal.size() != 32 * n) return 2;
    } else {
        if (!hex32(argv[4], tab[0]) || !hex32(argv[5], tab[1])) return 2;
        for (int j = 2; j < 65; ++j) tab[j] = fe_sqr<FrParams>(tab[j - 1]);
        start = strtoull(argv[6], nullptr, 10);
    }
    std::vector<uint8_t> out(sz * n + 1), inf(n + 1);
    for (size_t i = 0; i < n; ++i) {
        Fr k;
        if (scalars) memcpy(k.l, &scal[32 * i], 32);
        else k = pm::power_of(tab[0], tab + 1, start + i);
        if (!pm::below_r(k)) return 3;
        k = fe_from_mont<FrParams>(k);
        uint32_t row[pm::ROW_WORDS], w[48], o[48];
        pm::row_of(k.l, row);
        if ((row[3] | row[7]) >> 31) return 4;  // both magnitudes below 2^127
        memcpy(w, &recs[sz * i], sz);
        inf[i] = g2 ? pm::mul_point<pm::PmG2<sc::ScFp28>>(w, row, o) : pm::mul_point<pm::PmG1<sc::ScFp28>>(w, row, o);
        memcpy(&out[sz * i], o, sz);
    }
    printf("inf ");
    for (size_t i = 0; i < n; ++i) printf("%d", inf[i]);
    printf("\nout ");
    for (size_t i = 0; i < sz * n; ++i) printf("%02x", out[i]);
    printf("\n");
    return 0;
}
