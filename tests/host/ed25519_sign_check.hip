// Stand-alone CPU check of the Ed25519 signer's per-lane functions (bazuka_amd/csrc/bzk_ed25519_sign.cuh): the same __host__ __device__ code the
// gfx950 kernels run per lane, with the field's and the reduction's bound assertions on, built with the address and undefined-behaviour
// sanitizers and run by tests/test_ed25519_sign_cpu.py as a child process.  The expected values come from the test, made with Python integers:
//
//   ed25519_sign_check --muladd FILE    rows "k a r want" (64 hex digits each, most significant first): sc_muladd(k, a, r) == want
//   ed25519_sign_check --encode FILE    rows "k enc" (k as above, enc the 32 bytes in order): base_mul_encode(k) == enc
//
// and, with every run, the clamp at all-ones and all-zero digests.
#define BZK_FP28_CHECK 1
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bazuka_amd/csrc/bzk_ed25519_sign.cuh"

using namespace bzk;

static bool hex_bytes(const char* s, uint8_t* out, int n) {  // 2 n digits, in order
    for (int i = 0; i < n; ++i) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
// a 256-bit integer written most significant digit first, as eight little-endian words
static bool hex_int(const char* s, uint32_t (&w)[8]) {
    uint8_t be[32], le[32];
    if (strlen(s) != 64 || !hex_bytes(s, be, 32)) return false;
    for (int i = 0; i < 32; ++i) le[i] = be[31 - i];
    memcpy(w, le, 32);
    return true;
}

static int check_clamp() {
    uint32_t a[8];
    for (int i = 0; i < 8; ++i) a[i] = 0xffffffffu;
    ed25519::clamp(a);
    bool ok = a[0] == 0xfffffff8u && a[7] == 0x7fffffffu;
    for (int i = 1; i < 7; ++i) ok = ok && a[i] == 0xffffffffu;  // 2^255 - 8
    for (int i = 0; i < 8; ++i) a[i] = 0;
    ed25519::clamp(a);
    ok = ok && a[7] == 0x40000000u;  // 2^254
    for (int i = 0; i < 7; ++i) ok = ok && a[i] == 0;
    if (!ok) {
        printf("clamp: wrong\n");
        return 1;
    }
    printf("clamp ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (check_clamp()) return 1;
    if (argc != 3) return 0;
    const std::string mode = argv[1];
    FILE* f = fopen(argv[2], "r");
    if (!f) {
        printf("cannot open %s\n", argv[2]);
        return 2;
    }
    char c0[80], c1[80], c2[80], c3[80];
    int rows = 0;
    if (mode == "--muladd") {
        while (fscanf(f, "%79s %79s %79s %79s", c0, c1, c2, c3) == 4) {
            uint32_t k[8], a[8], r[8], want[8], got[8];
            if (!hex_int(c0, k) || !hex_int(c1, a) || !hex_int(c2, r) || !hex_int(c3, want)) {
                printf("row %d: not four 64-digit integers\n", rows);
                return 2;
            }
            ed25519::sc_muladd(k, a, r, got);
            if (memcmp(got, want, 32) != 0 || !ed25519::sc_below_l(got)) {
                printf("row %d: sc_muladd(%s, %s, %s) differs\n", rows, c0, c1, c2);
                return 1;
            }
            ++rows;
        }
    } else if (mode == "--encode") {
        std::vector<uint32_t> tab;
        ed25519::base_table_build(tab);
        while (fscanf(f, "%79s %79s", c0, c1) == 2) {
            uint32_t k[8], got[8];
            uint8_t want[32];
            if (!hex_int(c0, k) || strlen(c1) != 64 || !hex_bytes(c1, want, 32)) {
                printf("row %d: not an integer and 32 bytes\n", rows);
                return 2;
            }
            ed25519::base_mul_encode(k, tab.data(), got);
            if (memcmp(got, want, 32) != 0) {
                printf("row %d: base_mul_encode(%s) differs\n", rows, c0);
                return 1;
            }
            ++rows;
        }
    } else {
        printf("unknown mode %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    printf("%d rows ok\n", rows);
    return 0;
}
