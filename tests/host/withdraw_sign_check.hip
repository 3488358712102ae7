// Stand-alone check of the withdrawal producer's host code (bazuka_amd/csrc/bzk_withdraw_sign.cuh) without a GPU: the per-lane function
// withdraw_sign_one - the same __host__ __device__ text the gfx950 kernel runs per lane, with the bound assertions of the 29-bit field on - and
// the scatter that writes signatures and calldata into the records, built with the address and undefined-behaviour sanitizers (host code only)
// and run by tests/test_withdraw_sign_cpu.py as a child process.  The Poseidon constants come from libbzk.so's host table.
//   usage: _withdraw_sign_check FILE      FILE = u64 n, n x 128 key bytes, u64 len, len bytes of n bincode(MpnWithdraw) records
// For every byte alignment 0 .. 7 the records are copied into a heap block that ends with their last byte (a read or write past them is the
// sanitizer's to report), parsed, signed record by record and scattered into a second block of the same shape.  The eight outputs must be
// equal; they are printed once, as hex: "ok ...", "fp ...", "out ..." for the pytest side to compare with what Python integers give.
#define BZK_FP28_CHECK 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bazuka_amd/csrc/bzk_withdraw_sign.cuh"
#include "../../bazuka_amd/csrc/host_bincode.h"

namespace bzk {
int32_t poseidon_consts_host29(int t, const Fr29** out, int* rf, int* rp);  // poseidon.hip (libbzk.so): host memory, no device
}
using namespace bzk;

#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); \
            fprintf(stderr, __VA_ARGS__);               \
            fprintf(stderr, "\n");                      \
            exit(1);                                    \
        }                                               \
    } while (0)

static void put_hex(const char* what, const std::vector<uint8_t>& b) {
    printf("%s ", what);
    for (uint8_t v : b) printf("%02x", v);
    printf("\n");
}

int main(int argc, char** argv) {
    CHECK(argc == 2, "usage: %s FILE", argv[0]);
    FILE* f = fopen(argv[1], "rb");
    CHECK(f, "cannot open %s", argv[1]);
    uint64_t n = 0, len = 0;
    CHECK(fread(&n, 8, 1, f) == 1 && n >= 1 && n <= 4096, "count");
    std::vector<uint8_t> keys(n * 128);
    CHECK(fread(keys.data(), 1, keys.size(), f) == keys.size(), "keys");
    CHECK(fread(&len, 8, 1, f) == 1 && len >= 1 && len <= ((uint64_t)1 << 26), "length");
    std::vector<uint8_t> recs(len);
    CHECK(fread(recs.data(), 1, len, f) == len, "records");
    fclose(f);

    std::vector<Fr29> tab;
    eddsa::base_table_build(tab);
    eddsa::WithdrawSignConsts c;
    CHECK(poseidon_consts_host29(3, &c.c3, &c.rf3, &c.rp3) == 0 && poseidon_consts_host29(6, &c.c6, &c.rf6, &c.rp6) == 0 &&
              poseidon_consts_host29(7, &c.c7, &c.rf7, &c.rp7) == 0, "no Poseidon constants");
    c.tab = tab.data();

    std::vector<uint8_t> first_out, first_ok, first_fp;
    for (size_t a = 0; a < 8; ++a) {
        uint8_t* in = (uint8_t*)malloc(a + len);   // the records end with the block
        uint8_t* out = (uint8_t*)malloc(a + len);
        CHECK(in && out, "malloc");
        memcpy(in + a, recs.data(), len);
        memset(out, 0xEE, a + len);
        WdParsed P;
        std::string err;
        CHECK(parse_withdraws(in + a, len, n, P, err), "alignment %zu: %s", a, err.c_str());
        const WdSoA t = P.soa();
        std::vector<uint8_t> sig(n * 96), cd(n * 32), ok(n), fp(n * 32);
        for (uint64_t i = 0; i < n; ++i)
            ok[i] = eddsa::withdraw_sign_record_host(t, i, &keys[128 * i], c, &sig[96 * i], &cd[32 * i], &fp[32 * i]);
        CHECK(eddsa::withdraw_sign_scatter(t, n, sig.data(), cd.data(), ok.data(), out + a), "alignment %zu: an offset outside its record", a);
        for (size_t k = 0; k < a; ++k) CHECK(out[k] == 0xEE, "alignment %zu: a write before the records", a);
        const std::vector<uint8_t> got(out + a, out + a + len);
        if (a == 0) {
            first_out = got;
            first_ok = ok;
            first_fp = fp;
        }
        CHECK(got == first_out && ok == first_ok && fp == first_fp, "alignment %zu gives other bytes than alignment 0", a);
        // in place: the output block is the input block
        CHECK(eddsa::withdraw_sign_scatter(t, n, sig.data(), cd.data(), ok.data(), in + a), "alignment %zu in place", a);
        CHECK(memcmp(in + a, first_out.data(), len) == 0, "alignment %zu: in place gives other bytes", a);
        free(in);
        free(out);
    }
    put_hex("ok", first_ok);
    put_hex("fp", first_fp);
    put_hex("out", first_out);
    printf("eight alignments ok\n");
    return 0;
}
