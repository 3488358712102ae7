// The per-point subgroup checks (bazuka_amd/csrc/bzk_subgroup.cuh: g1_verdict, g2_verdict) in their DEVICE-field instantiation (sg::SgFp28: the
// 14 x 28-bit field, every product inlined), run on the CPU with the bound assertions of bzk_fp28.cuh on.  A stand-alone program, built with the
// address and undefined-behaviour sanitizers (host code only):
//     _subgroup_check g1|g2 <records file>
// reads n raw records (96 / 192 B each) and prints their n verdict digits on one line; tests/test_subgroup_cpu.py compares them with [r] P == identity
// from the oracle.  An assertion (an operand outside the bounds the field documents) aborts.
#define BZK_FP28_CHECK 1
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../bazuka_amd/csrc/bzk_subgroup.cuh"

using namespace bzk;

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[1], "g1") && strcmp(argv[1], "g2"))) {
        fprintf(stderr, "usage: %s g1|g2 <records file>\n", argv[0]);
        return 2;
    }
    const bool g2 = !strcmp(argv[1], "g2");
    const size_t sz = g2 ? 192 : 96;
    FILE* f = fopen(argv[2], "rb");
    if (!f) {
        perror(argv[2]);
        return 2;
    }
    std::vector<uint8_t> bytes;
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + k);
    fclose(f);
    if (bytes.size() % sz) {
        fprintf(stderr, "%zu bytes are not a whole number of %zu-byte records\n", bytes.size(), sz);
        return 2;
    }
    const size_t n = bytes.size() / sz;
    std::vector<char> out(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w[48];
        memcpy(w, bytes.data() + sz * i, sz);
        out[i] = (char)('0' + (g2 ? sg::g2_verdict<sg::SgFp28>(w) : sg::g1_verdict<sg::SgFp28>(w)));
    }
    printf("verdicts %s\n", out.data());
    return 0;
}
