// The wallet's side of a wire-form MpnWithdraw, one record per lane (withdraw_sign.hip mpn_withdraw_sign_kernel; the ctx = NULL route and the CPU
// harness tests/host/withdraw_sign_check.hip run the same code): the reference's `TxBuilder::withdraw_mpn` (src/wallet/tx_builder.rs:376-425)
//     fingerprint = ZkScalar::new(sha3_256(bincode(payment with calldata := 0)))     src/core/transaction.rs:204-211 (bzk_keccak.cuh, its own launch)
//     msg         = Poseidon(fingerprint, nonce)                                      :183-189
//     sig         = JubJub::sign(sk, msg)                                             bzk_eddsa_sign.cuh sign_one
//     calldata    = Poseidon(pk.x, pk.y, nonce, sig.r.x, sig.r.y, sig.s)              :177-182
// The three hang together in that order only: the message needs the payment's hash, the calldata needs the signature, the payment carries the
// calldata (which is why the fingerprint reads it as zeros).  As in sign_one the fixed-base walk indexes a table by nibbles of the secret nonce:
// fixed-flow, not address-independent - a throughput signer, not a hardened one.
//
// Field products per record (squares counted as products):
//   msg = Poseidon, arity 2        as sign_one's first hash, about                                               610
//   sign_one                       bzk_eddsa_sign.cuh, about                                                   3 000
//   calldata = Poseidon, arity 6   8 full rounds x (21 + 49) + 57 partial x 16 + 36 tail + 7 conversions, about 1 500     total about 5 100
// and, apart from them, one Keccak permutation per 136 payment bytes + one for the fingerprint.
#pragma once
#include <string.h>

#include "bzk_eddsa_sign.cuh"
#include "bzk_mpn_wire.h"

namespace bzk {
namespace eddsa {

// what a lane needs beside its own record: the sparse Poseidon constants of widths 3, 6 and 7 and the table of multiples of BASE
struct WithdrawSignConsts {
    const Fr29 *c3, *c6, *c7, *tab;
    int rf3, rp3, rf6, rp6, rf7, rp7;
};

// One withdrawal.  key = pub.x | pub.y | randomness | scalar, (addr_x, addr_odd) = the record's mpn_address, fingerprint = payment.fingerprint()
// (always a residue's limbs: ZkScalar::new made it); sig = r.x | r.y | s and calldata as Montgomery-256 limbs.  Returns 0, with zeros in sig and
// calldata, where a key field is not the limbs of a residue or the address is not the compression of pub.  Such a lane runs on zeros to the end:
// sign_one does that by itself for a key it refuses, and is handed a message it refuses (2^256 - 1) where only the address is wrong.
// key is read from memory three times (here, in sign_one, for the calldata) instead of being carried across the walk.
BZK_HD uint8_t withdraw_sign_one(const Fr* __restrict__ key, const Fr& addr_x, bool addr_odd, uint32_t nonce, const Fr& fingerprint,
                                 const WithdrawSignConsts& c, Fr* __restrict__ sig, Fr* __restrict__ calldata) {
    bool fit = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) fit = fit && canonical(key[i]);
    const Fr z = Fr::zero();
    {
        const Fr pub[2] = {fr_sel(fit, key[0], z), fr_sel(fit, key[1], z)};
        fit = fit && compresses_to(pub, addr_x, addr_odd);
    }
    Fr n = z;
    n.l[0] = nonce;
    Fr msg;
    {
        const Fr in[2] = {fr_sel(fit, fingerprint, z), fr_sel(fit, fe_to_mont<FrParams>(n), z)};
        msg = poseidon29_hash<3>(in, c.c3, c.rf3, c.rp3);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) msg.l[i] = fit ? msg.l[i] : 0xffffffffu;
    const bool ok = sign_one(key, &msg, c.c3, c.rf3, c.rp3, c.c6, c.rf6, c.rp6, c.tab, sig) != 0;
    BZK_EDDSA_OPAQUE(key);
    const Fr in[6] = {fr_sel(ok, key[0], z), fr_sel(ok, key[1], z), fr_sel(ok, fe_to_mont<FrParams>(n), z), sig[0], sig[1], sig[2]};
    calldata[0] = fr_sel(ok, poseidon29_hash<7>(in, c.c7, c.rf7, c.rp7), z);
    return ok ? 1 : 0;
}

// Record i of a parsed batch on the host, bytes in and bytes out (no buffer needs an alignment): its fingerprint always, its signature and
// calldata where the verdict is 1 (zeros otherwise)
inline uint8_t withdraw_sign_record_host(const WdSoA& t, uint64_t i, const uint8_t* key128, const WithdrawSignConsts& c, uint8_t sig96[96],
                                         uint8_t calldata32[32], uint8_t fingerprint32[32]) {
    Fr k[4], x, s[3], cd;
    memcpy(k, key128, 128);
    memcpy(&x, t.key_x + 32 * i, 32);
    const Fr fp = keccak::fr_from_le_bytes_mod(keccak::sha3_256_one(t.txs + t.pay_off[i], t.pay_len[i], t.cd_off[i]));
    const uint8_t ok = withdraw_sign_one(k, x, t.key_odd[i] != 0, t.nonce[i], fp, c, s, &cd);
    memcpy(sig96, s, 96);
    memcpy(calldata32, &cd, 32);
    memcpy(fingerprint32, &fp, 32);
    return ok;
}

// Writes the signed records: txs_out[0 .. rec_off[n]) = the input, then for every record with ok[i] != 0 its mpn_sig (the 96 bytes before the
// payment: mpn_address 33, nonce 4, signature) and its payment.calldata (32 bytes at pay_off + cd_off) replaced.  The only host code of the
// producer that writes at computed offsets: both ranges lie inside record i for anything parse_withdraws accepted (pay_off = rec_off + 133,
// cd_off + 32 <= pay_len, pay_off + pay_len = rec_off[i + 1]); a record that breaks that is left alone and reported.  txs_out may be the input.
inline bool withdraw_sign_scatter(const WdSoA& t, uint64_t n, const uint8_t* sig, const uint8_t* calldata, const uint8_t* ok, uint8_t* txs_out) {
    if (txs_out != t.txs) memmove(txs_out, t.txs, t.rec_off[n]);
    bool inside = true;
    for (uint64_t i = 0; i < n; ++i) {
        if (!ok[i]) continue;
        const uint64_t begin = t.rec_off[i], end = t.rec_off[i + 1], pay = t.pay_off[i];
        if (pay < begin + 96 || pay > end || (uint64_t)t.cd_off[i] + 32 > end - pay) {
            inside = false;
            continue;
        }
        memcpy(txs_out + pay - 96, sig + 96 * i, 96);
        memcpy(txs_out + pay + t.cd_off[i], calldata + 32 * i, 32);
    }
    return inside;
}

}  // namespace eddsa
}  // namespace bzk
