// The per-point scaling (bazuka_amd/csrc/bzk_scale.cuh: scale_point, recode) in its DEVICE-field instantiation (sc::ScFp28: the 14 x 28-bit field,
// every product inlined, Fermat's inversion), run on the CPU with the bound assertions of bzk_fp28.cuh on.  A stand-alone program, built with the
// address and undefined-behaviour sanitizers (host code only):
//     _scale_check <records file> <k: 64 hex digits, the 32 bytes of a Montgomery Fr scalar>
// reads n raw 96-byte records and prints "inf <n digits>" and "out <192 n hex digits>"; tests/test_params_rekey_cpu.py compares them with the oracle's
// products.  An assertion (an operand outside the bounds the field documents) aborts.
#define BZK_FP28_CHECK 1
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../bazuka_amd/csrc/bzk_scale.cuh"

using namespace bzk;

int main(int argc, char** argv) {
    if (argc != 3 || strlen(argv[2]) != 64) {
        fprintf(stderr, "usage: %s <records file> <k: 64 hex digits>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> recs;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) recs.insert(recs.end(), buf, buf + got);
    fclose(f);
    if (recs.size() % 96) return 2;
    uint8_t kb[32];
    for (int i = 0; i < 32; ++i) {
        unsigned v = 0;
        if (sscanf(argv[2] + 2 * i, "%2x", &v) != 1) return 2;
        kb[i] = (uint8_t)v;
    }
    Fr k;
    memcpy(k.l, kb, 32);
    sc::Digits dg;
    sc::recode(k, dg);
    const size_t n = recs.size() / 96;
    std::vector<uint8_t> out(96 * n + 1), inf(n + 1);
    for (size_t i = 0; i < n; ++i) {
        uint32_t w[24], o[24];
        memcpy(w, &recs[96 * i], 96);
        inf[i] = sc::scale_point<sc::ScFp28>(w, dg.w, o);
        memcpy(&out[96 * i], o, 96);
    }
    printf("inf ");
    for (size_t i = 0; i < n; ++i) printf("%d", inf[i]);
    printf("\nout ");
    for (size_t i = 0; i < 96 * n; ++i) printf("%02x", out[i]);
    printf("\n");
    return 0;
}
