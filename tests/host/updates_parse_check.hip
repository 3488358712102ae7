// Stand-alone harness of the ContractUpdate parser (bazuka_amd/csrc/host_bincode.h parse_contract_updates): built with the address and
// undefined-behaviour sanitizers (host code only) and run by tests/test_contract_updates_cpu.py as a child process.  The input file holds case
// records (u32 count, then u32 length + bytes each).  Every record is parsed whole, as every one of its prefixes, and with every byte raised by
// one and set to 0xff in turn (which covers each length word and each enum / Option tag); each buffer is a heap block of exactly its length, so
// a read past the input is the sanitizer's to report.  A parse may only answer "well-formed" or refuse with a message.
#include <stdio.h>
#include <stdlib.h>

#include "../../bazuka_amd/csrc/host_bincode.h"

using namespace bzk;

static uint64_t n_ok = 0, n_refused = 0;

static bool parse_block(const uint8_t* src, size_t len, const uint8_t cid[32], uint32_t flags) {
    uint8_t* block = (uint8_t*)malloc(len ? len : 1);
    if (!block) abort();
    memcpy(block, src, len);
    UpdParsed P;
    std::string err;
    const bool ok = parse_contract_updates(block, len, 1, flags, cid, P, err);
    if (ok) {
        // what a well-formed record hands on must lie inside it
        const upd::UpdRec& u = P.rec[0];
        if (u.at != 0 || (size_t)u.proof_off + upd::PROOF_BYTES != len || (size_t)u.commit_off + 48 > len || (size_t)u.next_off + 32 > len) abort();
        if ((size_t)u.pay0 + u.pay_n != P.pay.size()) abort();
        for (const upd::PayRec& p : P.pay) {
            if ((size_t)p.off + p.len > len || p.cd_off + 32 > p.len || p.src_off + 32 > p.len || p.amt_off + 12 > p.len || p.fee_off + 12 > p.len) abort();
            if ((p.flags & upd::PAY_HAS_SIG) && p.sig_off + 64 > p.len) abort();
            if (u.kind == upd::DEPOSIT && p.tag_off >= p.len) abort();
        }
        ++n_ok;
    } else {
        if (err.empty()) abort();  // a refusal names its reason
        ++n_refused;
    }
    free(block);
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> all;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + k);
    fclose(f);
    if (all.size() < 36) return 2;
    const uint8_t* cid = all.data();  // the file starts with the contract's 32 scalar bytes
    uint32_t count;
    memcpy(&count, all.data() + 32, 4);
    size_t at = 36;
    for (uint32_t c = 0; c < count; ++c) {
        uint32_t len;
        if (at + 4 > all.size()) return 2;
        memcpy(&len, all.data() + at, 4);
        at += 4;
        if (at + len > all.size()) return 2;
        const uint8_t* rec = all.data() + at;
        at += len;
        for (uint32_t flags = 0; flags < 2; ++flags) {
            const bool whole = parse_block(rec, len, cid, flags);
            if (flags == 0 && !whole) {
                fprintf(stderr, "case %u: the whole record is refused\n", c);
                return 1;
            }
            for (size_t k = 0; k < len; ++k)
                if (parse_block(rec, k, cid, flags)) {  // one record never ends early: a prefix that parses left bytes unread
                    fprintf(stderr, "case %u: prefix %zu parses\n", c, k);
                    return 1;
                }
            std::vector<uint8_t> m(rec, rec + len);
            for (size_t k = 0; k < len; ++k) {
                const uint8_t keep = m[k];
                m[k] = (uint8_t)(keep + 1);
                parse_block(m.data(), len, cid, flags);
                m[k] = 0xff;
                parse_block(m.data(), len, cid, flags);
                m[k] = keep;
            }
        }
    }
    printf("updates_parse_check: %u records, %llu parses well-formed, %llu refused\n", count, (unsigned long long)n_ok, (unsigned long long)n_refused);
    return 0;
}
