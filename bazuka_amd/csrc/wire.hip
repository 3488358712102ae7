// Wire-form admission: bincode records as the node receives them in, verdicts out, accepted ones queued into a world.  This file holds the
// extern "C" entry points of every wire-form path and, for the three MPN record kinds, the dispatcher that runs a parsed batch on the device
// (eddsa.hip mpn_*_verify_run) or - the same checks - on host threads.  The parsers are host_bincode.h's (structure only: byte ranges, integers,
// tags); the kernels and their orchestration are eddsa.hip's, updates.hip's and ed_sign.hip's.  No kernel lives here.
#include "bzk_ed25519_sign.h"  // the signing stage of bzk_mpn_deposits_sign / bzk_l1_txs_sign (ed_sign.hip)
#include "bzk_internal.h"
#include "host_bincode.h"
#include "host_mpn_world.h"  // struct bzk_mpn (the queues the push entry points fill), g_work_error
#include "host_threads.h"

using namespace bzk;

namespace bzk {
namespace {
std::atomic<uint32_t> g_wire_flags(0);  // bzk_mpn_set_wire_flags

bool limbs_of_a_residue(const uint8_t b[32]) {  // value < r (`from_repr` refuses anything else)
    uint32_t l[8];
    memcpy(l, b, 32);
    uint64_t borrow = 0;
    for (int i = 0; i < 8; ++i) borrow = (((uint64_t)l[i] - FrParams::MOD[i] - borrow) >> 63) & 1;
    return borrow != 0;
}
// PointCompressed::decompress with the reference's panic (no square root) and a non-residue's limbs reported as false
bool decompress_checked(const uint8_t x[32], bool odd, PointAffine& out) {
    out = PointAffine();
    if (!limbs_of_a_residue(x)) return false;
    const ZkScalar xs = ZkScalar::from_bytes(x), xx = xs.square();
    ZkScalar y;
    if (!((ZkScalar::one() - jubjub_d() * xx).invert() * (ZkScalar::one() + xx)).sqrt(&y)) return false;
    if (y.is_odd() != odd) y = -y;
    out = {xs, y};
    return true;
}
PointAffine point_at(const uint8_t xy[64]) { return {ZkScalar::from_bytes(xy), ZkScalar::from_bytes(xy + 32)}; }
JubjubSignature sig_at(const uint8_t s[96]) { return {point_at(s), ZkScalar::from_bytes(s + 64)}; }

// ------------------------------------------------------------------------------------------------
// Wire-form transactions: bincode(MpnTransaction) records in, signature verdicts out (bzk_mpn_tx_verify_batch), accepted ones queued
// (bzk_mpn_push_txs).
// ------------------------------------------------------------------------------------------------
// record i as it is queued, with its keys decompressed
MpnTx make_tx(const TxParsed& P, uint64_t i, const PointAffine& src, const PointAffine& dst) {
    MpnTx tx;
    tx.nonce = (uint32_t)P.nums[3 * i];
    tx.src_pub = src;
    tx.dst_pub = dst;
    tx.amount = Money{ZkScalar::from_bytes(&P.tok[64 * i]), P.nums[3 * i + 1]};
    tx.fee = Money{ZkScalar::from_bytes(&P.tok[64 * i + 32]), P.nums[3 * i + 2]};
    tx.sig = sig_at(&P.sig[96 * i]);
    return tx;
}
// record i on the host: the verdict, and the transaction with its keys decompressed (hash_ok: dst decompressed and the token ids are residues)
bool tx_verify_host(const TxParsed& P, uint64_t i, MpnTx& tx, bool& hash_ok) {
    PointAffine src, dst;
    const bool src_ok = decompress_checked(&P.src_x[32 * i], P.src_odd[i] != 0, src);
    const bool dst_ok = decompress_checked(&P.dst_x[32 * i], P.dst_odd[i] != 0, dst);
    hash_ok = dst_ok && limbs_of_a_residue(&P.tok[64 * i]) && limbs_of_a_residue(&P.tok[64 * i + 32]);
    bool sig_ok = true;
    for (int k = 0; k < 3; ++k) sig_ok = sig_ok && limbs_of_a_residue(&P.sig[96 * i + 32 * k]);
    tx = make_tx(P, i, src, dst);
    return src_ok && hash_ok && sig_ok && jubjub_verify(tx.src_pub, tx.hash(), tx.sig);
}
// all records: on the device when ctx is set, else on `threads` host threads.  txs_out (may be null): the transactions with decompressed keys
int32_t tx_verify_all(bzk_ctx* ctx, int threads, const TxParsed& P, uint64_t n, uint8_t* ok, uint8_t* hash_out, std::vector<MpnTx>* txs_out) {
    if (txs_out) txs_out->assign(n, MpnTx());
    if (ctx) {
        std::vector<uint8_t> sxy, dxy;
        if (txs_out) { sxy.resize(n * 64); dxy.resize(n * 64); }
        BZK_TRY(mpn_tx_verify_run(ctx, P.soa(), n, ok, hash_out, txs_out ? sxy.data() : nullptr, txs_out ? dxy.data() : nullptr));
        for (uint64_t i = 0; txs_out && i < n; ++i)
            if (ok[i]) (*txs_out)[i] = make_tx(P, i, point_at(&sxy[64 * i]), point_at(&dxy[64 * i]));  // only verified records are looked at again
        return BZK_OK;
    }
    host_for_each(n, threads, [&](uint64_t i) {
        MpnTx local;
        MpnTx& tx = txs_out ? (*txs_out)[i] : local;
        bool hash_ok;
        ok[i] = tx_verify_host(P, i, tx, hash_ok) ? 1 : 0;
        if (hash_out) {
            if (hash_ok) tx.hash().to_bytes(hash_out + 32 * i);
            else memset(hash_out + 32 * i, 0, 32);
        }
    });
    return BZK_OK;
}

// ------------------------------------------------------------------------------------------------
// Wire-form withdrawals: bincode(MpnWithdraw) records in, verdicts and fingerprints out (bzk_mpn_withdraw_verify_batch), accepted ones queued with
// their payment bytes (bzk_mpn_push_withdraws).
// ------------------------------------------------------------------------------------------------
// record i as it is queued, with its key decompressed and its payment's fingerprint
WithdrawTx make_withdraw(const WdParsed& P, uint64_t i, const PointAffine& key, const ZkScalar& fingerprint) {
    WithdrawTx tx;
    tx.mpn_address = key;
    tx.nonce = P.nonce[i];
    tx.sig = sig_at(&P.sig[96 * i]);
    tx.amount = Money{ZkScalar::from_bytes(&P.tok[64 * i]), P.amounts[2 * i]};
    tx.fee = Money{ZkScalar::from_bytes(&P.tok[64 * i + 32]), P.amounts[2 * i + 1]};
    tx.fingerprint = fingerprint;
    tx.payment.assign(P.txs + P.pay_off[i], P.txs + P.pay_off[i] + P.pay_len[i]);
    return tx;
}
// record i on the host: the two verdict bits, the fingerprint, and the withdrawal with its key decompressed
uint8_t withdraw_verify_host(const WdParsed& P, uint64_t i, WithdrawTx& tx) {
    PointAffine key;
    const bool key_ok = decompress_checked(&P.key_x[32 * i], P.key_odd[i] != 0, key);
    bool sig_ok = true;
    for (int k = 0; k < 3; ++k) sig_ok = sig_ok && limbs_of_a_residue(&P.sig[96 * i + 32 * k]);
    std::vector<uint8_t> blanked(P.txs + P.pay_off[i], P.txs + P.pay_off[i] + P.pay_len[i]);
    memset(blanked.data() + P.cd_off[i], 0, 32);
    tx = make_withdraw(P, i, key, hash_to_scalar(blanked.data(), blanked.size()));
    if (!key_ok || !sig_ok) return 0;
    uint8_t calldata[32];
    tx.calldata().to_bytes(calldata);
    return (uint8_t)((jubjub_verify(tx.mpn_address, tx.sign_message(), tx.sig) ? 1 : 0) |
                     (memcmp(calldata, tx.payment.data() + P.cd_off[i], 32) == 0 ? 2 : 0));
}
// all records: on the device when ctx is set, else on `threads` host threads.  out (may be null): the withdrawals as they would be queued
int32_t withdraw_verify_all(bzk_ctx* ctx, int threads, const WdParsed& P, uint64_t n, uint8_t* ok, uint8_t* fp_out, std::vector<WithdrawTx>* out) {
    if (out) out->assign(n, WithdrawTx());
    if (ctx) {
        std::vector<uint8_t> xy, fp;
        if (out) { xy.resize(n * 64); fp.resize(n * 32); }
        uint8_t* fpp = out ? fp.data() : fp_out;
        BZK_TRY(mpn_withdraw_verify_run(ctx, P.soa(), n, ok, fpp, out ? xy.data() : nullptr));
        if (out && fp_out) memcpy(fp_out, fp.data(), n * 32);
        for (uint64_t i = 0; out && i < n; ++i)
            if (ok[i] == 3) (*out)[i] = make_withdraw(P, i, point_at(&xy[64 * i]), ZkScalar::from_bytes(&fp[32 * i]));  // only admissible records are looked at again
        return BZK_OK;
    }
    host_for_each(n, threads, [&](uint64_t i) {
        WithdrawTx local;
        WithdrawTx& tx = out ? (*out)[i] : local;
        ok[i] = withdraw_verify_host(P, i, tx);
        if (fp_out) tx.fingerprint.to_bytes(fp_out + 32 * i);
    });
    return BZK_OK;
}

// ------------------------------------------------------------------------------------------------
// Wire-form deposits: bincode(MpnDeposit) records in, verdicts and decompressed addresses out (bzk_mpn_deposit_verify_batch), accepted ones queued
// with their payment bytes (bzk_mpn_push_deposits).  The Ed25519 check of ContractDeposit::verify_signature (src/core/transaction.rs:192-202) is
// eddsa.hip's, on the device or - the same per-lane code - on host threads.
// ------------------------------------------------------------------------------------------------
// record i as it is queued, with its address decompressed
DepositTx make_deposit(const DpParsed& P, uint64_t i, const PointAffine& address) {
    DepositTx tx;
    tx.mpn_address = address;
    tx.amount = Money{ZkScalar::from_bytes(&P.tok[32 * i]), P.amount[i]};
    tx.payment.assign(P.txs + P.pay_off[i], P.txs + P.pay_off[i] + P.pay_len[i]);
    return tx;
}
// all records: on the device when ctx is set, else on `threads` host threads; xy n x 64: the decompressed addresses (zeros where there is none)
int32_t deposit_verify_all(bzk_ctx* ctx, int threads, const DpParsed& P, uint64_t n, uint8_t* ok, uint8_t* xy) {
    if (ctx) return mpn_deposit_verify_run(ctx, P.soa(), n, ok, xy);
    const DpSoA t = P.soa();
    host_for_each(n, threads, [&](uint64_t i) {
        PointAffine a;
        const bool key_ok = decompress_checked(&P.key_x[32 * i], P.key_odd[i] != 0, a);
        ok[i] = (uint8_t)(mpn_deposit_sig_host(t, i) | (key_ok ? 2 : 0));
        if (xy) {
            a.x.to_bytes(xy + 64 * i);
            a.y.to_bytes(xy + 64 * i + 32);
        }
    });
    return BZK_OK;
}
// where signed record i is written: head bytes of the input, the tag, the optional length prefix, the signature, then the input from tail_at on
struct SignedSplice {
    uint64_t head_end, tail_at;  // in the input: the tag's position, and the first byte after the input's own signature field
};
// out_len, and with out set the records themselves: record i as it stands where ok[i] = 0, else spliced.  tag4: the tag is a u32 (an enum's), not a
// byte (an Option's)
uint64_t write_signed(const uint8_t* txs, const uint64_t* rec_off, const std::vector<SignedSplice>& at, const uint8_t* ok, const uint8_t* sig, uint64_t n,
                      bool tag4, uint32_t flags, uint8_t* out) {
    uint64_t pos = 0;
    auto put = [&](const void* p, uint64_t k) {
        if (out && k) memcpy(out + pos, p, k);
        pos += k;
    };
    for (uint64_t i = 0; i < n; ++i) {
        if (!ok[i]) {
            put(txs + rec_off[i], rec_off[i + 1] - rec_off[i]);
            continue;
        }
        const uint8_t tag[4] = {1, 0, 0, 0};
        const uint64_t len64 = 64;
        put(txs + rec_off[i], at[i].head_end - rec_off[i]);
        put(tag, tag4 ? 4 : 1);
        if (flags & BZK_WORK_SIG_LEN_PREFIXED) put(&len64, 8);
        put(sig + 64 * i, 64);
        put(txs + at[i].tail_at, rec_off[i + 1] - at[i].tail_at);
    }
    return pos;
}
}  // namespace

int32_t contract_updates_run(bzk_ctx* ctx, const bzk_contract_desc& c, UpdParsed& P, const uint64_t* count, uint64_t m, uint64_t height0,
                             const uint8_t state0[32], uint8_t* ok, uint8_t* aux_out, uint8_t* commit_out);  // updates.hip
}  // namespace bzk

extern "C" {

int32_t bzk_mpn_tx_verify_batch(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok, uint8_t* hash_out) {
    if (n && (!txs || !ok)) return BZK_E_ARG;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        TxParsed P;
        if (!parse_txs(txs, len, n, P, g_work_error)) return BZK_E_ARG;
        return tx_verify_all(ctx, host_default_threads(), P, n, ok, hash_out, nullptr);
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

int32_t bzk_mpn_push_txs(bzk_mpn* w, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok_out, uint64_t* accepted_out) {
    if (!w || (n && !txs)) return BZK_E_ARG;
    if (accepted_out) *accepted_out = 0;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        TxParsed P;
        if (!parse_txs(txs, len, n, P, g_work_error)) return BZK_E_ARG;
        std::vector<uint8_t> ok(n);
        std::vector<MpnTx> parsed;
        if (const int32_t st = tx_verify_all(w->dev, w->threads, P, n, ok.data(), nullptr, &parsed); st != BZK_OK) {
            if (w->dev) w->dev_error = bzk_last_error(w->dev);
            return st;
        }
        uint64_t accepted = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (!ok[i]) continue;
            w->mempool.push_back(parsed[i]);
            ++accepted;
        }
        if (ok_out) memcpy(ok_out, ok.data(), n);
        if (accepted_out) *accepted_out = accepted;
        return BZK_OK;
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

int32_t bzk_host_jubjub_decompress(const uint8_t x[32], int32_t odd, uint8_t xy_out[64]) {
    if (!x || !xy_out) return BZK_E_ARG;
    PointAffine p;
    const bool ok = decompress_checked(x, odd != 0, p);
    p.x.to_bytes(xy_out);
    p.y.to_bytes(xy_out + 32);
    return ok ? 1 : 0;
}

int32_t bzk_mpn_withdraw_verify_batch(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok, uint8_t* fingerprint_out) {
    if (n && (!txs || !ok)) return BZK_E_ARG;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        WdParsed P;
        if (!parse_withdraws(txs, len, n, P, g_work_error)) return BZK_E_ARG;
        return withdraw_verify_all(ctx, host_default_threads(), P, n, ok, fingerprint_out, nullptr);
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

int32_t bzk_mpn_push_withdraws(bzk_mpn* w, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok_out, uint64_t* accepted_out) {
    if (!w || (n && !txs)) return BZK_E_ARG;
    if (accepted_out) *accepted_out = 0;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        WdParsed P;
        if (!parse_withdraws(txs, len, n, P, g_work_error)) return BZK_E_ARG;
        std::vector<uint8_t> ok(n);
        std::vector<WithdrawTx> parsed;
        if (const int32_t st = withdraw_verify_all(w->dev, w->threads, P, n, ok.data(), nullptr, &parsed); st != BZK_OK) {
            if (w->dev) w->dev_error = bzk_last_error(w->dev);
            return st;
        }
        uint8_t world_id[32];
        w->contract_id.to_bytes(world_id);
        uint64_t accepted = 0;
        for (uint64_t i = 0; i < n; ++i) {
            // mempool.rs:246-258 for a withdrawal: the payment is for this contract's withdraw circuit 0 and signed; calldata as withdraw.rs:77 checks it
            const bool admit = ok[i] == 3 && memcmp(&P.cid[32 * i], world_id, 32) == 0 && P.circuit[i] == 0 &&
                               limbs_of_a_residue(&P.tok[64 * i]) && limbs_of_a_residue(&P.tok[64 * i + 32]);
            ok[i] = admit ? 1 : 0;
            if (!admit) continue;
            w->withdraw_queue.push_back(std::move(parsed[i]));
            ++accepted;
        }
        if (ok_out) memcpy(ok_out, ok.data(), n);
        if (accepted_out) *accepted_out = accepted;
        return BZK_OK;
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

int32_t bzk_mpn_set_wire_flags(uint32_t flags) {
    if (flags & ~BZK_WORK_SIG_LEN_PREFIXED) return BZK_E_ARG;
    g_wire_flags.store(flags);
    return BZK_OK;
}

int32_t bzk_mpn_deposit_verify_batch(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok, uint8_t* addr_xy_out) {
    if (n && (!txs || !ok)) return BZK_E_ARG;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        DpParsed P;
        if (!parse_deposits(txs, len, n, g_wire_flags.load(), P, g_work_error)) return BZK_E_ARG;
        return deposit_verify_all(ctx, host_default_threads(), P, n, ok, addr_xy_out);
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

int32_t bzk_mpn_push_deposits(bzk_mpn* w, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok_out, uint64_t* accepted_out) {
    if (!w || (n && !txs)) return BZK_E_ARG;
    if (accepted_out) *accepted_out = 0;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        DpParsed P;
        if (!parse_deposits(txs, len, n, g_wire_flags.load(), P, g_work_error)) return BZK_E_ARG;
        std::vector<uint8_t> ok(n), xy(n * 64);
        if (const int32_t st = deposit_verify_all(w->dev, w->threads, P, n, ok.data(), xy.data()); st != BZK_OK) {
            if (w->dev) w->dev_error = bzk_last_error(w->dev);
            return st;
        }
        uint8_t world_id[32];
        w->contract_id.to_bytes(world_id);
        uint64_t accepted = 0;
        for (uint64_t i = 0; i < n; ++i) {
            // mempool.rs:241-258 for a deposit: the payment is for this contract's deposit circuit 0 and signed; the address as apply_deposit.rs:8 needs it
            const bool admit = ok[i] == 3 && memcmp(&P.cid[32 * i], world_id, 32) == 0 && P.circuit[i] == 0 && limbs_of_a_residue(&P.tok[32 * i]);
            ok[i] = admit ? 1 : 0;
            if (!admit) continue;
            w->deposit_queue.push_back(make_deposit(P, i, point_at(&xy[64 * i])));
            ++accepted;
        }
        if (ok_out) memcpy(ok_out, ok.data(), n);
        if (accepted_out) *accepted_out = accepted;
        return BZK_OK;
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

// ------------------------------------------------------------------------------------------------
// Wire-form L1 transactions: bincode(Transaction) / bincode(TransactionAndDelta) records in, verify_signature verdicts and Transaction::hash out
// (bzk_l1_tx_verify_batch); whole block bodies in, per-block verdict and Merkle root out (bzk_block_bodies_check).  The parser is
// host_bincode.h's parse_l1_txs (structure only); hashing, Ed25519 and the trees are eddsa.hip's, on the device or on host threads.
// ------------------------------------------------------------------------------------------------
int32_t bzk_l1_tx_verify_batch(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, uint64_t n, uint32_t form, uint8_t* ok, uint8_t* hash_out) {
    if (form > BZK_L1_FORM_TX_AND_DELTA || (n && (!txs || !ok))) return BZK_E_ARG;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        L1Parsed P;
        if (!parse_l1_txs(txs, len, n, form == BZK_L1_FORM_TX_AND_DELTA, g_wire_flags.load(), P, g_work_error)) return BZK_E_ARG;
        if (ctx) return l1_check_run(ctx, P.soa(), n, nullptr, 0, ok, hash_out, nullptr, nullptr);
        return l1_check_host(host_default_threads(), P.soa(), n, nullptr, 0, ok, hash_out, nullptr, nullptr);
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

int32_t bzk_block_bodies_check(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, const uint64_t* count, uint64_t m, uint8_t* sig_ok_out,
                               uint8_t* root_out, uint8_t* tx_ok_out, uint8_t* hash_out) {
    if (m && (!count || !sig_ok_out || !root_out)) return BZK_E_ARG;
    if (m == 0 && len == 0) return BZK_OK;
    uint64_t n = 0;
    for (uint64_t j = 0; j < m; ++j) {
        if (count[j] > len) return BZK_E_ARG;  // a record is tens of bytes: also keeps the sum from wrapping
        n += count[j];
    }
    if (n && !txs) return BZK_E_ARG;
    try {
        L1Parsed P;
        if (!parse_l1_txs(txs, len, n, false, g_wire_flags.load(), P, g_work_error)) return BZK_E_ARG;
        if (ctx) return l1_check_run(ctx, P.soa(), n, count, m, tx_ok_out, hash_out, sig_ok_out, root_out);
        return l1_check_host(host_default_threads(), P.soa(), n, count, m, tx_ok_out, hash_out, sig_ok_out, root_out);
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

// ------------------------------------------------------------------------------------------------
// The producers of the two Ed25519-signed record kinds: `TxBuilder::sign_deposit` and `TxBuilder::sign_tx` (src/wallet/tx_builder.rs:63-70) for
// n records and n keys.  The parsers, and so the refusals, are the verify entries'; the signing is ed_sign.hip's, on the device or on host
// threads; this file writes the records back with their signature filled in, spelled as bzk_mpn_set_wire_flags says.
// ------------------------------------------------------------------------------------------------
int32_t bzk_mpn_deposits_sign(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* sig_out, uint8_t* ok,
                              uint8_t* txs_out, uint64_t cap, uint64_t* out_len) {
    if (n && (!keys || !txs || !sig_out || !ok)) return BZK_E_ARG;
    if (out_len) *out_len = 0;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        const uint32_t flags = g_wire_flags.load();
        DpParsed P;
        if (!parse_deposits(txs, len, n, flags, P, g_work_error)) return BZK_E_ARG;
        std::vector<uint8_t> sig(n * 64), verdict(n);
        BZK_TRY(mpn_deposits_sign_all(ctx, host_default_threads(), P.soa(), keys, n, sig.data(), verdict.data()));
        std::vector<SignedSplice> at(n);
        for (uint64_t i = 0; i < n; ++i) at[i] = {P.pay_off[i] + P.tag_off[i], P.pay_off[i] + P.pay_len[i]};
        const uint64_t need = write_signed(txs, P.rec_off.data(), at, verdict.data(), sig.data(), n, false, flags, nullptr);
        if (out_len) *out_len = need;
        if (txs_out && cap < need) {
            g_work_error = "txs_out holds " + std::to_string(cap) + " bytes, the signed records need " + std::to_string(need);
            return BZK_E_ARG;
        }
        memcpy(sig_out, sig.data(), n * 64);
        memcpy(ok, verdict.data(), n);
        if (txs_out) write_signed(txs, P.rec_off.data(), at, verdict.data(), sig.data(), n, false, flags, txs_out);
        return BZK_OK;
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

int32_t bzk_l1_txs_sign(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* txs, uint64_t len, uint64_t n, uint32_t form, uint8_t* sig_out, uint8_t* ok,
                        uint8_t* hash_out, uint8_t* txs_out, uint64_t cap, uint64_t* out_len) {
    if (form > BZK_L1_FORM_TX_AND_DELTA || (n && (!keys || !txs || !sig_out || !ok))) return BZK_E_ARG;
    if (out_len) *out_len = 0;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        const uint32_t flags = g_wire_flags.load();
        L1Parsed P;
        if (!parse_l1_txs(txs, len, n, form == BZK_L1_FORM_TX_AND_DELTA, flags, P, g_work_error)) return BZK_E_ARG;
        std::vector<uint8_t> sig(n * 64), verdict(n), hash(hash_out ? n * 32 : 0);
        BZK_TRY(l1_txs_sign_all(ctx, host_default_threads(), P.soa(), keys, n, sig.data(), verdict.data(), hash_out ? hash.data() : nullptr));
        std::vector<SignedSplice> at(n);
        for (uint64_t i = 0; i < n; ++i) {
            const l1::L1Rec& r = P.rec[i];
            at[i] = {P.rec_off[i] + r.sig_tag, P.rec_off[i] + ((r.flags & l1::SIGNED) ? r.sig_off + 64 : r.sig_tag + 4)};
        }
        const uint64_t need = write_signed(txs, P.rec_off.data(), at, verdict.data(), sig.data(), n, true, flags, nullptr);
        if (out_len) *out_len = need;
        if (txs_out && cap < need) {
            g_work_error = "txs_out holds " + std::to_string(cap) + " bytes, the signed records need " + std::to_string(need);
            return BZK_E_ARG;
        }
        memcpy(sig_out, sig.data(), n * 64);
        memcpy(ok, verdict.data(), n);
        if (hash_out) memcpy(hash_out, hash.data(), n * 32);
        if (txs_out) write_signed(txs, P.rec_off.data(), at, verdict.data(), sig.data(), n, true, flags, txs_out);
        return BZK_OK;
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

// ------------------------------------------------------------------------------------------------
// Wire-form ContractUpdates: bincode(ContractUpdate) records of one contract in, per-update verdict bits, aux data and commitments out
// (bzk_contract_updates_check); and the parse-only helper that cuts those records out of L1 transactions (bzk_l1_tx_updates).  The parser is
// host_bincode.h's parse_contract_updates (structure only); everything computed is updates.hip's, on the device or on host threads.
// ------------------------------------------------------------------------------------------------
int32_t bzk_contract_updates_check(bzk_ctx* ctx, const bzk_contract_desc* c, const uint8_t* updates, uint64_t len, const uint64_t* count, uint64_t m,
                                   uint64_t height0, const uint8_t state0[32], uint8_t* ok, uint8_t* aux_out, uint8_t* commit_out) {
    if (m && !count) {
        g_work_error = "count is NULL with transactions to check";
        return BZK_E_ARG;
    }
    uint64_t n = 0;
    for (uint64_t j = 0; j < m; ++j) {
        if (count[j] > len) {  // a record is hundreds of bytes: also keeps the sum from wrapping
            g_work_error = "the counts name more records than the input can hold";
            return BZK_E_ARG;
        }
        n += count[j];
    }
    if (n == 0 && len == 0) return BZK_OK;
    if (!c || (n && (!updates || !state0 || !ok))) {
        g_work_error = "a pointer is NULL with records to check";
        return BZK_E_ARG;
    }
    if ((c->n_deposit_fns && !c->deposit_fns) || (c->n_withdraw_fns && !c->withdraw_fns) || (c->n_fns && !c->fns)) {
        g_work_error = "a function table is NULL with a non-zero count";
        return BZK_E_ARG;
    }
    const bzk_contract_fn* tab[3] = {c->deposit_fns, c->withdraw_fns, c->fns};
    const uint32_t cnt[3] = {c->n_deposit_fns, c->n_withdraw_fns, c->n_fns};
    for (int t = 0; t < 3; ++t)
        for (uint32_t k = 0; k < cnt[t]; ++k) {
            if (!tab[t][k].vk || tab[t][k].vk_len < 878) {
                g_work_error = "function " + std::to_string(k) + ": a verifying key is at least 878 bytes";
                return BZK_E_ARG;
            }
            if (t < 2 && tab[t][k].log4_payment_capacity > upd::MAX_CAPACITY) {
                g_work_error = "function " + std::to_string(k) + ": log4_payment_capacity above 8";
                return BZK_E_ARG;
            }
        }
    try {
        UpdParsed P;
        if (!parse_contract_updates(updates, len, n, g_wire_flags.load(), c->contract_id, P, g_work_error)) return BZK_E_ARG;
        return contract_updates_run(ctx, *c, P, count, m, height0, state0, ok, aux_out, commit_out);
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

int32_t bzk_l1_tx_updates(const uint8_t* txs, uint64_t len, uint64_t n, uint32_t form, const uint8_t contract_id[32], uint64_t* spans_out, uint64_t cap,
                          uint64_t* n_out) {
    if (form > BZK_L1_FORM_TX_AND_DELTA || !contract_id || !n_out || (n && !txs) || (cap && !spans_out)) return BZK_E_ARG;
    *n_out = 0;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        L1Parsed P;
        UpdSpans S;
        S.cid = contract_id;
        if (!parse_l1_txs(txs, len, n, form == BZK_L1_FORM_TX_AND_DELTA, g_wire_flags.load(), P, g_work_error, &S)) return BZK_E_ARG;
        const uint64_t found = S.out.size() / 3;
        if (found && cap) memcpy(spans_out, S.out.data(), (size_t)std::min(found, cap) * 24);
        *n_out = found;
        return BZK_OK;
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

int32_t bzk_l1_tx_deltas(const uint8_t* txs, uint64_t len, uint64_t n, uint32_t form, const uint8_t contract_id[32], uint64_t* spans_out, uint64_t cap,
                         uint64_t* n_out) {
    if (form > BZK_L1_FORM_TX_AND_DELTA || !contract_id || !n_out || (n && !txs) || (cap && !spans_out)) return BZK_E_ARG;
    *n_out = 0;
    if (n == 0 && len == 0) return BZK_OK;
    try {
        L1Parsed P;
        UpdSpans S;
        S.cid = contract_id;
        if (!parse_l1_txs(txs, len, n, form == BZK_L1_FORM_TX_AND_DELTA, g_wire_flags.load(), P, g_work_error, &S)) return BZK_E_ARG;
        const uint64_t found = S.deltas.size() / 4;
        if (found && cap) memcpy(spans_out, S.deltas.data(), (size_t)std::min(found, cap) * 32);
        *n_out = found;
        return BZK_OK;
    } catch (const std::bad_alloc&) {
        return BZK_E_ALLOC;
    }
}

}  // extern "C"
