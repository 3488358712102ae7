// The producer of wire-form MpnWithdraw records (bzk_mpn_withdraws_sign): `TxBuilder::withdraw_mpn` (src/wallet/tx_builder.rs:376-425) for n
// records and n keys.  The parser, and so the refusals, are bzk_mpn_withdraw_verify_batch's; the fingerprints come from eddsa.hip's SHA3 launch;
// the arithmetic is bzk_withdraw_sign.cuh's withdraw_sign_one.  This file holds the one kernel that chains message hash, signature and calldata
// hash per lane, its orchestration and the entry point.  ctx = NULL runs the same per-lane function on host threads.

// as in sign.hip: the hashes share a kernel with the fixed-base walk, so their MDS matrix is re-read in every full round
#define BZK_POSEIDON_MDS_RELOAD 1
#include <mutex>

#include "bzk_withdraw_sign.cuh"
#include "bzk_internal.h"
#include "bzk_stage.h"
#include "host_bincode.h"
#include "host_mpn_world.h"  // g_work_error
#include "host_threads.h"

namespace bzk {

int32_t poseidon_consts_dev_shared(bzk_ctx* ctx, int t, const void** out, int* rf, int* rp);  // poseidon.hip
int32_t poseidon_consts_host29(int t, const Fr29** out, int* rf, int* rp);                    // poseidon.hip
int32_t eddsa_table_dev(bzk_ctx* ctx, const Fr29** out);                                      // eddsa.hip

// One wave per block and no LDS, for jubjub_sign_kernel's reasons (sign.hip): a record is one dependent chain - hash, walk and inversion, hash,
// hash - of some five thousand products, so the only parallelism is across lanes.  One launch stands for six (hash inputs, arity-2 Poseidon,
// signer, second inputs, arity-6 Poseidon, verdict) and for the arrays between them: the message and the six calldata inputs never leave the lane.
// The width-7 hash starts after sign_one's state is dead, so the register peak is the signer's.
constexpr int WD_SIGN_BLOCK = 64;
__global__ void __launch_bounds__(WD_SIGN_BLOCK) mpn_withdraw_sign_kernel(const Fr* __restrict__ keys, const Fr* __restrict__ addr_x,
                                                                          const uint8_t* __restrict__ addr_odd, const uint32_t* __restrict__ nonce,
                                                                          const Fr* __restrict__ fp, uint64_t m, eddsa::WithdrawSignConsts c,
                                                                          Fr* __restrict__ sig, Fr* __restrict__ calldata, uint8_t* __restrict__ ok) {
    const uint64_t i = (uint64_t)blockIdx.x * WD_SIGN_BLOCK + threadIdx.x;
    if (i >= m) return;
    Fr s[3], cd;
    ok[i] = eddsa::withdraw_sign_one(keys + 4 * i, addr_x[i], addr_odd[i] != 0, nonce[i], fp[i], c, s, &cd);
#pragma unroll
    for (int k = 0; k < 3; ++k) sig[3 * i + k] = s[k];
    calldata[i] = cd;
}

namespace {

int32_t consts_dev(bzk_ctx* ctx, eddsa::WithdrawSignConsts& c) {
    const void *p3, *p6, *p7;
    BZK_TRY(poseidon_consts_dev_shared(ctx, 3, &p3, &c.rf3, &c.rp3));
    BZK_TRY(poseidon_consts_dev_shared(ctx, 6, &p6, &c.rf6, &c.rp6));
    BZK_TRY(poseidon_consts_dev_shared(ctx, 7, &p7, &c.rf7, &c.rp7));
    c.c3 = (const Fr29*)p3;
    c.c6 = (const Fr29*)p6;
    c.c7 = (const Fr29*)p7;
    return eddsa_table_dev(ctx, &c.tab);
}
int32_t consts_host(eddsa::WithdrawSignConsts& c) {  // the table is built once
    static std::once_flag once;
    static std::vector<Fr29> tab;
    std::call_once(once, [] { eddsa::base_table_build(tab); });
    BZK_TRY(poseidon_consts_host29(3, &c.c3, &c.rf3, &c.rp3));
    BZK_TRY(poseidon_consts_host29(6, &c.c6, &c.rf6, &c.rp6));
    BZK_TRY(poseidon_consts_host29(7, &c.c7, &c.rf7, &c.rp7));
    c.tab = tab.data();
    return BZK_OK;
}

// n parsed records and n keys on the device.  Rounds are cut as mpn_withdraw_verify_run cuts them (MPN_TX_CHUNK records or MPN_WD_CHUNK_BYTES of
// payment bytes, whichever comes first); a round's records go up as they stand and the SHA3 launch indexes the payments inside them.  Per round:
// the fingerprints (sha3_256_launch with the calldata blanked, then ZkScalar::new), then the signing kernel.  sig n x 96, calldata n x 32, ok n,
// fp_out n x 32 or null (host memory).  No hashing and no field arithmetic on the host.  The staged key bytes are overwritten before the call
// returns.
int32_t mpn_withdraws_sign_run(bzk_ctx* ctx, const WdSoA& t, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* calldata, uint8_t* ok,
                               uint8_t* fp_out) {
    if (n == 0) return BZK_OK;
    (void)hipSetDevice(ctx->device);
    Stage<StreamOps> st({ctx}, "mpn_withdraws_sign_run", n, MPN_TX_CHUNK, MPN_WD_CHUNK_BYTES, [&](uint64_t i) { return (uint64_t)t.pay_len[i]; }, t.rec_off);
    std::vector<uint64_t> begin = round_bases(st.round_at, t.rec_off), end(n);  // payment ranges relative to their round's first byte
    for (uint64_t i = 0; i < n; ++i) {
        begin[i] = t.pay_off[i] - begin[i];
        end[i] = begin[i] + t.pay_len[i];
    }
    uint8_t *dbytes, *dbeg, *dend, *dcd, *dnonce, *dkeys, *dkx, *dodd, *dfp, *dsig, *dcall, *dok;
    st.bytes(dbytes, t.txs, 0, 0); st.in(dbeg, begin.data(), 8); st.in(dend, end.data(), 8); st.in(dcd, t.cd_off, 4); st.in(dnonce, t.nonce, 4);
    st.in(dkeys, keys, 128); st.in(dkx, t.key_x, 32); st.in(dodd, t.key_odd, 1); st.out(dfp, fp_out, 32); st.out(dsig, sig, 96);
    st.out(dcall, calldata, 32); st.out(dok, ok, 1);
    st.wipe(dkeys, st.cap * 128);  // the staged keys do not outlive the call
    BZK_TRY(st.ws.commit(ctx));
    eddsa::WithdrawSignConsts k;
    BZK_TRY(consts_dev(ctx, k));
    return st.run([&](uint64_t, uint64_t m) {
        BZK_TRY(sha3_256_launch(ctx, dbytes, dbeg, dend, 0, dcd, m, nullptr, dfp));
        BZK_LAUNCH(ctx, "mpn_withdraw_sign", mpn_withdraw_sign_kernel, dim3((unsigned)((m + WD_SIGN_BLOCK - 1) / WD_SIGN_BLOCK)), dim3(WD_SIGN_BLOCK), 0,
                   (const Fr*)dkeys, (const Fr*)dkx, (const uint8_t*)dodd, (const uint32_t*)dnonce, (const Fr*)dfp, m, k, (Fr*)dsig, (Fr*)dcall, dok);
        return BZK_OK;
    });
}
// the same per-lane function on host threads
int32_t mpn_withdraws_sign_host(int threads, const WdSoA& t, const uint8_t* keys, uint64_t n, uint8_t* sig, uint8_t* calldata, uint8_t* ok,
                                uint8_t* fp_out) {
    eddsa::WithdrawSignConsts k;
    BZK_TRY(consts_host(k));
    host_for_each(n, threads, [&](uint64_t i) {
        uint8_t fp[32];
        ok[i] = eddsa::withdraw_sign_record_host(t, i, keys + 128 * i, k, sig + 96 * i, calldata + 32 * i, fp);
        if (fp_out) memcpy(fp_out + 32 * i, fp, 32);
    });
    return BZK_OK;
}

}  // namespace
}  // namespace bzk

using namespace bzk;

extern "C" {

int32_t bzk_mpn_withdraws_sign(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* txs_out, uint8_t* ok,
                               uint8_t* fingerprint_out) {
    if (n && (!keys || !txs || !txs_out || !ok)) return BZK_E_ARG;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        WdParsed P;
        if (!parse_withdraws(txs, len, n, P, g_work_error)) return BZK_E_ARG;
        std::vector<uint8_t> sig(n * 96), calldata(n * 32);
        const WdSoA t = P.soa();
        if (ctx) BZK_TRY(mpn_withdraws_sign_run(ctx, t, keys, n, sig.data(), calldata.data(), ok, fingerprint_out));
        else BZK_TRY(mpn_withdraws_sign_host(host_default_threads(), t, keys, n, sig.data(), calldata.data(), ok, fingerprint_out));
        if (!eddsa::withdraw_sign_scatter(t, n, sig.data(), calldata.data(), ok, txs_out)) {
            g_work_error = "bzk_mpn_withdraws_sign: a parsed record's offsets lie outside it";
            return BZK_E_INTERNAL;
        }
        return BZK_OK;
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

}  // extern "C"
