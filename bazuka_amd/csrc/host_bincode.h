// f-2: the prover's wire format.  `MpnWork` (src/mpn/mod.rs:263-270) is what a proving worker receives
// from `GET /bincode/mpn/work` (src/node/mod.rs:393-398, src/client/messages.rs:368-376) and `ZkProof`
// (src/zk/mod.rs:646-651) is what it posts back; both travel as bincode 1.3.3 with the default options the reference
// uses everywhere (`bincode::serialize` / `deserialize`): little-endian fixed-width integers, u64 sequence / string /
// map lengths, u32 enum variant indices, `Option` as one tag byte, tuples / fixed arrays / `PhantomData` without any
// framing.  The layouts below restate the reference's `#[derive(Serialize)]` type definitions field by field:
//
//   MpnWork            { config, public_inputs, data, new_root, reward }                      src/mpn/mod.rs:263-270
//   MpnConfig          { 5 x u8 log4 sizes, mpn_contract_id, 3 x usize batch counts, 3 x ZkVerifierKey }   :202-216
//   ZkPublicInputs     { height u64, state, aux_data, next_state }                                          :250-256
//   MpnWorkData        enum { Deposit(Vec<..>) = 0, Withdraw(Vec<..>) = 1, Update(Vec<..>) = 2 }             :243-248
//   {Deposit,Withdraw,Update}Transition                                                                     :426-511
//   MpnAccount         { tx_nonce u32, withdraw_nonce u32, address PointAffine, tokens HashMap<u64, Money> } src/zk/mod.rs:59-65
//   MpnTransaction     { nonce u32, src_pub_key, dst_pub_key (PointCompressed = ZkScalar + bool), amount, fee, sig }  :584-593
//   ZkCompressedState  { state_hash, state_size u64 }                                                       :542-546
//   ZkVerifierKey      enum { Groth16(Box<Groth16VerifyingKey>) = 0 }   (the 1460-byte blobs of src/config/blockchain.rs:32-37)
//   Money { token_id: ContractId, amount: Amount(u64) }; ContractId enum { Null = 0, Ziesha = 1, Custom(ZkScalar) = 2 }
//                                                                                      src/core/transaction.rs:60-81
//   MpnDeposit { mpn_address, payment: ContractDeposit }, MpnWithdraw { mpn_address, mpn_withdraw_nonce, mpn_sig, payment }
//   ContractDeposit / ContractWithdraw (L1 payments)                                                        :136-174
//   ZkScalar = 4 x u64 Montgomery limbs (`#[derive(Serialize)] struct ZkScalar([u64; 4])`, src/zk/mod.rs:202-206)
//
// Two leaf types come from crates that are not vendored (Cargo.toml:31 `ed25519-dalek = "1"`, no lockfile) [recalled]:
// `ed25519_dalek::PublicKey` serialises as a byte string (u64 length 32 + 32 bytes) and `ed25519::Signature` as a
// 64-element tuple (64 bytes, no length; releases before ed25519 1.3 wrote a length-prefixed byte string - selectable
// with BZK_WORK_SIG_LEN_PREFIXED).  They only occur inside the L1 payments of deposit / withdraw works, which the
// circuits read three fields of; the payment is otherwise carried as an opaque byte range.
//
// The reference holds no golden `MpnWork` payloads (parity unpinned for this format too); what IS pinned
// is the `ZkVerifierKey` encoding (the hard-coded verifying keys), which this codec round-trips byte for byte
// (tests/test_work_codec_cpu.py), and every scalar type it is built from (Poseidon KATs on the Montgomery limbs).
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "bzk_l1.h"
#include "bzk_mpn_wire.h"
#include "bzk_updates.h"
#include "host_mpn_types.h"

namespace bzk {

#ifndef BZK_WORK_SIG_LEN_PREFIXED
#define BZK_WORK_SIG_LEN_PREFIXED 1u  // include/bzk.h
#endif

struct BinReader {
    const uint8_t* p;
    size_t n, pos = 0;
    bool ok = true;
    std::string err;
    BinReader(const uint8_t* d, size_t len) : p(d), n(len) {}
    bool fail(const char* what) {
        if (ok) {
            ok = false;
            err = std::string(what) + " at byte " + std::to_string(pos);
        }
        return false;
    }
    bool need(size_t k, const char* what) { return (ok && n - pos >= k) ? true : fail(what); }
    uint8_t u8(const char* what = "u8") {
        if (!need(1, what)) return 0;
        return p[pos++];
    }
    bool boolean(const char* what = "bool") {
        const uint8_t v = u8(what);
        if (ok && v > 1) fail("bool is neither 0 nor 1");  // bincode rejects other values
        return v == 1;
    }
    uint32_t u32(const char* what = "u32") {
        if (!need(4, what)) return 0;
        uint32_t v;
        memcpy(&v, p + pos, 4);
        pos += 4;
        return v;
    }
    uint64_t u64(const char* what = "u64") {
        if (!need(8, what)) return 0;
        uint64_t v;
        memcpy(&v, p + pos, 8);
        pos += 8;
        return v;
    }
    const uint8_t* bytes(size_t k, const char* what = "bytes") {
        if (!need(k, what)) return nullptr;
        const uint8_t* r = p + pos;
        pos += k;
        return r;
    }
    ZkScalar scalar(const char* what = "ZkScalar") {
        const uint8_t* b = bytes(32, what);
        return b ? ZkScalar::from_bytes(b) : ZkScalar();
    }
    uint64_t len(size_t min_elem_bytes, const char* what) {  // a sequence length that the remaining input can hold
        const uint64_t v = u64(what);
        if (ok && min_elem_bytes && v > (n - pos) / min_elem_bytes) fail(what);
        return ok ? v : 0;
    }
};

struct BinWriter {
    std::vector<uint8_t> b;
    void u8(uint8_t v) { b.push_back(v); }
    void u32(uint32_t v) { raw(&v, 4); }
    void u64(uint64_t v) { raw(&v, 8); }
    void raw(const void* d, size_t k) {
        const uint8_t* s = (const uint8_t*)d;
        b.insert(b.end(), s, s + k);
    }
    void scalar(const ZkScalar& s) {
        uint8_t t[32];
        s.to_bytes(t);
        raw(t, 32);
    }
};

// ---- scalars and small composites ---------------------------------------------------------------
// ContractId <-> the scalar the circuits use (`impl From<ContractId> for ZkScalar`, src/zk/mod.rs:280-288)
inline ZkScalar rd_contract_id(BinReader& r) {
    const uint32_t tag = r.u32("ContractId tag");
    if (tag == 0) return ZkScalar::zero();
    if (tag == 1) return ZkScalar::one();
    if (tag == 2) return r.scalar("ContractId::Custom");
    r.fail("ContractId variant");
    return ZkScalar();
}
inline void wr_contract_id(BinWriter& w, const ZkScalar& id) {  // `impl From<ZkScalar> for ContractId`, transaction.rs:97-107
    if (id.is_zero()) return w.u32(0);
    if (id == ZkScalar::one()) return w.u32(1);
    w.u32(2);
    w.scalar(id);
}
inline Money rd_money(BinReader& r) {
    Money m;
    m.token_id = rd_contract_id(r);
    m.amount = r.u64("Amount");
    return m;
}
inline void wr_money(BinWriter& w, const Money& m) {
    wr_contract_id(w, m.token_id);
    w.u64(m.amount);
}
inline PointAffine rd_point(BinReader& r) {
    PointAffine p;
    p.x = r.scalar("PointAffine.0");
    p.y = r.scalar("PointAffine.1");
    return p;
}
inline void wr_point(BinWriter& w, const PointAffine& p) {
    w.scalar(p.x);
    w.scalar(p.y);
}
// jubjub::PublicKey(PointCompressed(x, y_is_odd)); the circuits allocate its decompression (curve.rs:78-88, which
// `unwrap`s the square root: an x that is not on the curve is rejected here instead of panicking)
inline PointAffine rd_pubkey(BinReader& r) {
    const ZkScalar x = r.scalar("PointCompressed.0");
    const bool odd = r.boolean("PointCompressed.1");
    if (!r.ok) return PointAffine();
    PointAffine p = jubjub_decompress(x, odd);
    if (!p.is_on_curve()) r.fail("PointCompressed does not decompress");
    return p;
}
inline void wr_pubkey(BinWriter& w, const PointAffine& p) {  // PointAffine::compress (curve.rs:70-74)
    w.scalar(p.x);
    w.u8(p.y.is_odd() ? 1 : 0);
}
inline JubjubSignature rd_zksig(BinReader& r) {
    JubjubSignature s;
    s.r = rd_point(r);
    s.s = r.scalar("Signature.s");
    return s;
}
inline void wr_zksig(BinWriter& w, const JubjubSignature& s) {
    wr_point(w, s.r);
    w.scalar(s.s);
}
inline Proof4 rd_proof(BinReader& r, const char* what) {
    const uint64_t k = r.len(96, what);
    Proof4 p((size_t)k);
    for (uint64_t i = 0; i < k && r.ok; ++i)
        for (int j = 0; j < 3; ++j) p[(size_t)i][j] = r.scalar(what);
    return p;
}
inline void wr_proof(BinWriter& w, const Proof4& p) {
    w.u64(p.size());
    for (auto& t : p)
        for (int j = 0; j < 3; ++j) w.scalar(t[j]);
}
inline MpnAccount rd_account(BinReader& r) {
    MpnAccount a;
    a.tx_nonce = r.u32("MpnAccount.tx_nonce");
    a.withdraw_nonce = r.u32("MpnAccount.withdraw_nonce");
    a.address = rd_point(r);
    const uint64_t k = r.len(20, "MpnAccount.tokens");
    for (uint64_t i = 0; i < k && r.ok; ++i) {
        const uint64_t key = r.u64("token index");
        a.tokens[key] = rd_money(r);
    }
    return a;
}
inline void wr_account(BinWriter& w, const MpnAccount& a) {  // HashMap order is unspecified on the wire: ascending here
    w.u32(a.tx_nonce);
    w.u32(a.withdraw_nonce);
    wr_point(w, a.address);
    w.u64(a.tokens.size());
    for (auto& kv : a.tokens) {
        w.u64(kv.first);
        wr_money(w, kv.second);
    }
}
inline MpnTx rd_mpn_tx(BinReader& r) {
    MpnTx t;
    t.nonce = r.u32("MpnTransaction.nonce");
    t.src_pub = rd_pubkey(r);
    t.dst_pub = rd_pubkey(r);
    t.amount = rd_money(r);
    t.fee = rd_money(r);
    t.sig = rd_zksig(r);
    return t;
}
inline void wr_mpn_tx(BinWriter& w, const MpnTx& t) {
    w.u32(t.nonce);
    wr_pubkey(w, t.src_pub);
    wr_pubkey(w, t.dst_pub);
    wr_money(w, t.amount);
    wr_money(w, t.fee);
    wr_zksig(w, t.sig);
}

// ---- L1 payments (opaque except for amount / fee and, for withdrawals, the fingerprint) ---------------------------
inline void skip_string(BinReader& r) {
    const uint64_t k = r.len(1, "String length");
    r.bytes((size_t)k, "String");
}
inline void skip_l1_pub(BinReader& r) {  // ed25519_dalek::PublicKey: byte string of 32
    if (r.u64("ed25519 public key length") != 32) r.fail("ed25519 public key length");
    r.bytes(32, "ed25519 public key");
}
// ContractDeposit { memo, contract_id, deposit_circuit_id, calldata, src, amount, fee, nonce, sig: Option<Sig> }
inline void rd_contract_deposit(BinReader& r, uint32_t flags, DepositTx& tx) {
    const size_t p0 = r.pos;
    skip_string(r);
    rd_contract_id(r);
    r.u32("deposit_circuit_id");
    r.scalar("calldata");
    skip_l1_pub(r);
    tx.amount = rd_money(r);
    rd_money(r);  // fee: paid on L1, not seen by the circuit
    r.u32("nonce");
    const uint8_t some = r.u8("Option<Signature> tag");
    if (r.ok && some > 1) r.fail("Option tag");
    if (r.ok && some) {
        if (flags & BZK_WORK_SIG_LEN_PREFIXED)
            if (r.u64("ed25519 signature length") != 64) r.fail("ed25519 signature length");
        r.bytes(64, "ed25519 signature");
    }
    if (r.ok) tx.payment.assign(r.p + p0, r.p + r.pos);
}
// ContractWithdraw { memo, contract_id, withdraw_circuit_id, calldata, dst, amount, fee }
// fingerprint = ZkScalar::new(sha3(bincode(payment with calldata := 0)))  (transaction.rs:204-211)
inline void rd_contract_withdraw(BinReader& r, WithdrawTx& tx) {
    const size_t p0 = r.pos;
    skip_string(r);
    rd_contract_id(r);
    r.u32("withdraw_circuit_id");
    const size_t calldata_at = r.pos;
    r.scalar("calldata");
    skip_l1_pub(r);
    tx.amount = rd_money(r);
    tx.fee = rd_money(r);
    if (!r.ok) return;
    tx.payment.assign(r.p + p0, r.p + r.pos);
    std::vector<uint8_t> unsigned_bin = tx.payment;
    memset(unsigned_bin.data() + (calldata_at - p0), 0, 32);
    tx.fingerprint = hash_to_scalar(unsigned_bin.data(), unsigned_bin.size());
}
// the payment a synthetic world attaches to a queued deposit / withdrawal (tests, benches): empty memo, circuit 0,
// zero calldata, an all-zero L1 key, no L1 signature
inline std::vector<uint8_t> default_contract_deposit(const ZkScalar& contract_id, const Money& amount) {
    BinWriter w;
    w.u64(0);
    wr_contract_id(w, contract_id);
    w.u32(0);
    w.scalar(ZkScalar());
    w.u64(32);
    const uint8_t z[32] = {0};
    w.raw(z, 32);
    wr_money(w, amount);
    wr_money(w, Money{ZkScalar::one(), 0});
    w.u32(0);
    w.u8(0);
    return w.b;
}
inline std::vector<uint8_t> default_contract_withdraw(const ZkScalar& contract_id, const Money& amount, const Money& fee,
                                                      const ZkScalar& calldata) {
    BinWriter w;
    w.u64(0);
    wr_contract_id(w, contract_id);
    w.u32(0);
    w.scalar(calldata);
    w.u64(32);
    const uint8_t z[32] = {0};
    w.raw(z, 32);
    wr_money(w, amount);
    wr_money(w, fee);
    return w.b;
}
inline ZkScalar contract_withdraw_fingerprint(const std::vector<uint8_t>& payment) {  // calldata sits after memo + id + u32
    BinReader r(payment.data(), payment.size());
    skip_string(r);
    rd_contract_id(r);
    r.u32();
    if (!r.ok || payment.size() < r.pos + 32) return ZkScalar();
    std::vector<uint8_t> u = payment;
    memset(u.data() + r.pos, 0, 32);
    return hash_to_scalar(u.data(), u.size());
}

// ---- transitions ------------------------------------------------------------------------------------------------
inline DepositTransition rd_deposit_transition(BinReader& r, uint32_t flags) {
    DepositTransition t;
    t.enabled = r.boolean("DepositTransition.enabled");
    t.tx.mpn_address = rd_pubkey(r);
    rd_contract_deposit(r, flags, t.tx);
    t.before = rd_account(r);
    t.before_balances_hash = r.scalar("before_balances_hash");
    t.before_balance = rd_money(r);
    t.proof = rd_proof(r, "proof");
    t.account_index = r.u64("account_index");
    t.token_index = r.u64("token_index");
    t.balance_proof = rd_proof(r, "balance_proof");
    return t;
}
inline void wr_deposit_transition(BinWriter& w, const DepositTransition& t, const ZkScalar& contract_id) {
    w.u8(t.enabled ? 1 : 0);
    wr_pubkey(w, t.tx.mpn_address);
    const std::vector<uint8_t> pay = t.tx.payment.empty() ? default_contract_deposit(contract_id, t.tx.amount) : t.tx.payment;
    w.raw(pay.data(), pay.size());
    wr_account(w, t.before);
    w.scalar(t.before_balances_hash);
    wr_money(w, t.before_balance);
    wr_proof(w, t.proof);
    w.u64(t.account_index);
    w.u64(t.token_index);
    wr_proof(w, t.balance_proof);
}
inline WithdrawTransition rd_withdraw_transition(BinReader& r) {
    WithdrawTransition t;
    t.enabled = r.boolean("WithdrawTransition.enabled");
    t.tx.mpn_address = rd_pubkey(r);
    t.tx.nonce = r.u32("mpn_withdraw_nonce");
    t.tx.sig = rd_zksig(r);
    rd_contract_withdraw(r, t.tx);
    t.before = rd_account(r);
    t.before_token_balance = rd_money(r);
    t.before_fee_balance = rd_money(r);
    t.proof = rd_proof(r, "proof");
    t.account_index = r.u64("account_index");
    t.token_index = r.u64("token_index");
    t.token_balance_proof = rd_proof(r, "token_balance_proof");
    t.before_token_hash = r.scalar("before_token_hash");
    t.fee_token_index = r.u64("fee_token_index");
    t.fee_balance_proof = rd_proof(r, "fee_balance_proof");
    return t;
}
inline void wr_withdraw_transition(BinWriter& w, const WithdrawTransition& t) {
    w.u8(t.enabled ? 1 : 0);
    wr_pubkey(w, t.tx.mpn_address);
    w.u32(t.tx.nonce);
    wr_zksig(w, t.tx.sig);
    w.raw(t.tx.payment.data(), t.tx.payment.size());  // never empty: see bzk_mpn_push_withdraw / the decoder
    wr_account(w, t.before);
    wr_money(w, t.before_token_balance);
    wr_money(w, t.before_fee_balance);
    wr_proof(w, t.proof);
    w.u64(t.account_index);
    w.u64(t.token_index);
    wr_proof(w, t.token_balance_proof);
    w.scalar(t.before_token_hash);
    w.u64(t.fee_token_index);
    wr_proof(w, t.fee_balance_proof);
}
inline UpdateTransition rd_update_transition(BinReader& r) {
    UpdateTransition t;
    t.enabled = r.boolean("UpdateTransition.enabled");
    t.tx = rd_mpn_tx(r);
    t.src_before = rd_account(r);
    t.src_before_balances_hash = r.scalar("src_before_balances_hash");
    t.src_before_balance = rd_money(r);
    t.src_before_fee_balance = rd_money(r);
    t.src_proof = rd_proof(r, "src_proof");
    t.src_index = r.u64("src_index");
    t.src_token_index = r.u64("src_token_index");
    t.src_balance_proof = rd_proof(r, "src_balance_proof");
    t.src_fee_token_index = r.u64("src_fee_token_index");
    t.src_fee_balance_proof = rd_proof(r, "src_fee_balance_proof");
    t.dst_before = rd_account(r);
    t.dst_before_balances_hash = r.scalar("dst_before_balances_hash");
    t.dst_before_balance = rd_money(r);
    t.dst_proof = rd_proof(r, "dst_proof");
    t.dst_index = r.u64("dst_index");
    t.dst_token_index = r.u64("dst_token_index");
    t.dst_balance_proof = rd_proof(r, "dst_balance_proof");
    return t;
}
inline void wr_update_transition(BinWriter& w, const UpdateTransition& t) {
    w.u8(t.enabled ? 1 : 0);
    wr_mpn_tx(w, t.tx);
    wr_account(w, t.src_before);
    w.scalar(t.src_before_balances_hash);
    wr_money(w, t.src_before_balance);
    wr_money(w, t.src_before_fee_balance);
    wr_proof(w, t.src_proof);
    w.u64(t.src_index);
    w.u64(t.src_token_index);
    wr_proof(w, t.src_balance_proof);
    w.u64(t.src_fee_token_index);
    wr_proof(w, t.src_fee_balance_proof);
    wr_account(w, t.dst_before);
    w.scalar(t.dst_before_balances_hash);
    wr_money(w, t.dst_before_balance);
    wr_proof(w, t.dst_proof);
    w.u64(t.dst_index);
    w.u64(t.dst_token_index);
    wr_proof(w, t.dst_balance_proof);
}

// ---- MpnConfig / MpnWork ------------------------------------------------------------------------------------------
// Groth16VerifyingKey: alpha_g1, beta_g1 (97 B each), beta_g2, gamma_g2 (193), delta_g1 (97), delta_g2 (193),
// ic: Vec<97 B>  (src/zk/groth16/mod.rs:22-31; 870 + 8 + 97 * ic.len() bytes, 1460 for the MPN circuits' 6 entries)
inline std::vector<uint8_t> rd_verifier_key(BinReader& r) {
    if (r.u32("ZkVerifierKey tag") != 0) r.fail("ZkVerifierKey variant (only Groth16 = 0 exists outside cfg(test))");
    const size_t p0 = r.pos;
    r.bytes(870, "Groth16VerifyingKey points");
    const uint64_t k = r.len(97, "Groth16VerifyingKey.ic");
    r.bytes((size_t)k * 97, "Groth16VerifyingKey.ic");
    return r.ok ? std::vector<uint8_t>(r.p + p0, r.p + r.pos) : std::vector<uint8_t>();
}
inline bool verifier_key_well_formed(const std::vector<uint8_t>& vk) {
    if (vk.size() < 878) return false;
    uint64_t k;
    memcpy(&k, vk.data() + 870, 8);
    return k <= (vk.size() - 878) / 97 && vk.size() == 878 + 97 * (size_t)k;
}
struct MpnWorkConfig {
    uint8_t log4_tree = 0, log4_token_tree = 0, log4_deposit_batch = 0, log4_withdraw_batch = 0, log4_update_batch = 0;
    ZkScalar mpn_contract_id;
    uint64_t num_update_batches = 0, num_deposit_batches = 0, num_withdraw_batches = 0;
    std::vector<uint8_t> deposit_vk, withdraw_vk, update_vk;  // bincode(Groth16VerifyingKey), without the enum tag
};
struct MpnWork {
    MpnWorkConfig config;
    uint64_t height = 0;
    ZkScalar state, aux_data, next_state;
    int kind = 2;  // MpnWorkData variant index: 0 Deposit, 1 Withdraw, 2 Update
    std::vector<DepositTransition> deposits;
    std::vector<WithdrawTransition> withdraws;
    std::vector<UpdateTransition> updates;
    ZkScalar new_root_hash;
    uint64_t new_root_size = 0;
    uint64_t reward = 0;
    size_t n_transitions() const { return kind == 0 ? deposits.size() : kind == 1 ? withdraws.size() : updates.size(); }
    int log4_batch() const {
        return kind == 0 ? config.log4_deposit_batch : kind == 1 ? config.log4_withdraw_batch : config.log4_update_batch;
    }
    const std::vector<uint8_t>& vk() const {  // MpnWork::vk (src/mpn/mod.rs:273-280)
        return kind == 0 ? config.deposit_vk : kind == 1 ? config.withdraw_vk : config.update_vk;
    }
};

inline bool mpn_work_decode(BinReader& r, uint32_t flags, MpnWork& w) {
    MpnWorkConfig& c = w.config;
    c.log4_tree = r.u8("log4_tree_size");
    c.log4_token_tree = r.u8("log4_token_tree_size");
    c.log4_deposit_batch = r.u8("log4_deposit_batch_size");
    c.log4_withdraw_batch = r.u8("log4_withdraw_batch_size");
    c.log4_update_batch = r.u8("log4_update_batch_size");
    c.mpn_contract_id = rd_contract_id(r);
    c.num_update_batches = r.u64("mpn_num_update_batches");
    c.num_deposit_batches = r.u64("mpn_num_deposit_batches");
    c.num_withdraw_batches = r.u64("mpn_num_withdraw_batches");
    c.deposit_vk = rd_verifier_key(r);
    c.withdraw_vk = rd_verifier_key(r);
    c.update_vk = rd_verifier_key(r);
    w.height = r.u64("public_inputs.height");
    w.state = r.scalar("public_inputs.state");
    w.aux_data = r.scalar("public_inputs.aux_data");
    w.next_state = r.scalar("public_inputs.next_state");
    const uint32_t tag = r.u32("MpnWorkData tag");
    if (r.ok && tag > 2) r.fail("MpnWorkData variant");
    w.kind = (int)tag;
    const uint64_t k = r.len(1, "transitions");
    for (uint64_t i = 0; i < k && r.ok; ++i) {
        if (tag == 0) w.deposits.push_back(rd_deposit_transition(r, flags));
        else if (tag == 1) w.withdraws.push_back(rd_withdraw_transition(r));
        else w.updates.push_back(rd_update_transition(r));
    }
    w.new_root_hash = r.scalar("new_root.state_hash");
    w.new_root_size = r.u64("new_root.state_size");
    w.reward = r.u64("reward");
    return r.ok;
}
inline void mpn_work_encode(BinWriter& o, const MpnWork& w) {
    const MpnWorkConfig& c = w.config;
    o.u8(c.log4_tree);
    o.u8(c.log4_token_tree);
    o.u8(c.log4_deposit_batch);
    o.u8(c.log4_withdraw_batch);
    o.u8(c.log4_update_batch);
    wr_contract_id(o, c.mpn_contract_id);
    o.u64(c.num_update_batches);
    o.u64(c.num_deposit_batches);
    o.u64(c.num_withdraw_batches);
    for (const std::vector<uint8_t>* vk : {&c.deposit_vk, &c.withdraw_vk, &c.update_vk}) {
        o.u32(0);
        o.raw(vk->data(), vk->size());
    }
    o.u64(w.height);
    o.scalar(w.state);
    o.scalar(w.aux_data);
    o.scalar(w.next_state);
    o.u32((uint32_t)w.kind);
    o.u64(w.n_transitions());
    for (auto& t : w.deposits) wr_deposit_transition(o, t, c.mpn_contract_id);
    for (auto& t : w.withdraws) wr_withdraw_transition(o, t);
    for (auto& t : w.updates) wr_update_transition(o, t);
    o.scalar(w.new_root_hash);
    o.u64(w.new_root_size);
    o.u64(w.reward);
}

// commitment of a solution: ZkScalar::new(sha3_256(bincode((prover, reward))))  (MpnWork::verify, src/mpn/mod.rs:281-295)
// prover = the worker's L1 address (ed25519 public key: byte string of 32), reward = Amount(u64)
inline ZkScalar mpn_work_commitment(const uint8_t prover_pub[32], uint64_t reward) {
    BinWriter w;
    w.u64(32);
    w.raw(prover_pub, 32);
    w.u64(reward);
    return hash_to_scalar(w.b.data(), w.b.size());
}

// ---- wire-form MPN records (bzk_mpn_wire.h): structure only --------------------------------------------------------------------------------
// parse_txs / parse_withdraws / parse_deposits cut n consecutive bincode(MpnTransaction) / bincode(MpnWithdraw) / bincode(MpnDeposit) records into
// the arrays the device stages (TxSoA / WdSoA / DpSoA).  They only cut byte ranges, read integers and tags and map ContractId tags: no hashing
// and no field arithmetic, so that the device paths (eddsa.hip mpn_*_verify_run) leave none on the host.
struct TxParsed {
    std::vector<uint8_t> src_x, dst_x, src_odd, dst_odd, tok, sig;
    std::vector<uint64_t> nums, rec_end;  // rec_end n: where record i ends in the input (its signature is the 96 bytes before)
    TxSoA soa() const { return {src_x.data(), dst_x.data(), src_odd.data(), dst_odd.data(), tok.data(), nums.data(), sig.data()}; }
};
// ContractId as the scalar the circuits use, copied as bytes (Null = 0, Ziesha = 1: constants)
inline void parse_contract_id(BinReader& r, uint8_t out[32]) {
    const uint32_t tag = r.u32("ContractId tag");
    memset(out, 0, 32);
    if (tag == 0) return;
    if (tag == 1) return ZkScalar::one().to_bytes(out);
    if (tag == 2) {
        if (const uint8_t* b = r.bytes(32, "ContractId::Custom")) memcpy(out, b, 32);
        return;
    }
    r.fail("ContractId variant");
}
inline bool parse_txs(const uint8_t* txs, uint64_t len, uint64_t n, TxParsed& P, std::string& err) {
    if (n > len / 190) {  // the shortest record: 4 + 2 x 33 + 2 x 12 + 96
        err = "fewer bytes than " + std::to_string(n) + " MpnTransaction records need";
        return false;
    }
    P.src_x.resize(n * 32); P.dst_x.resize(n * 32); P.src_odd.resize(n); P.dst_odd.resize(n);
    P.tok.resize(n * 64); P.sig.resize(n * 96); P.nums.resize(n * 3); P.rec_end.resize(n);
    BinReader r(txs, (size_t)len);
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        P.nums[3 * i] = r.u32("MpnTransaction.nonce");
        if (const uint8_t* b = r.bytes(32, "PointCompressed.0")) memcpy(&P.src_x[32 * i], b, 32);
        P.src_odd[i] = r.boolean("PointCompressed.1") ? 1 : 0;
        if (const uint8_t* b = r.bytes(32, "PointCompressed.0")) memcpy(&P.dst_x[32 * i], b, 32);
        P.dst_odd[i] = r.boolean("PointCompressed.1") ? 1 : 0;
        parse_contract_id(r, &P.tok[64 * i]);
        P.nums[3 * i + 1] = r.u64("Amount");
        parse_contract_id(r, &P.tok[64 * i + 32]);
        P.nums[3 * i + 2] = r.u64("Amount");
        if (const uint8_t* b = r.bytes(96, "Signature")) memcpy(&P.sig[96 * i], b, 96);
        P.rec_end[i] = r.pos;
        if (!r.ok) r.err = "record " + std::to_string(i) + ": " + r.err;
    }
    if (r.ok && r.pos != len) r.fail("bytes after the last record");
    err = r.err;
    return r.ok;
}
struct WdParsed {
    const uint8_t* txs = nullptr;
    std::vector<uint64_t> rec_off, pay_off, amounts;  // amounts n x 2: amount, fee
    std::vector<uint32_t> pay_len, cd_off, nonce, circuit;
    std::vector<uint8_t> key_x, key_odd, sig, cid, tok;  // cid n x 32: payment.contract_id as a scalar; tok n x 64: amount | fee token ids
    WdSoA soa() const {
        return {txs, rec_off.data(), pay_off.data(), pay_len.data(), cd_off.data(), key_x.data(), key_odd.data(), nonce.data(), sig.data()};
    }
};
inline bool parse_withdraws(const uint8_t* txs, uint64_t len, uint64_t n, WdParsed& P, std::string& err) {
    if (n > len / 245) {  // the shortest record: 33 + 4 + 96 + (8 + 4 + 4 + 32 + 40 + 2 x 12)
        err = "fewer bytes than " + std::to_string(n) + " MpnWithdraw records need";
        return false;
    }
    P.txs = txs;
    P.rec_off.resize(n + 1); P.pay_off.resize(n); P.amounts.resize(2 * n);
    P.pay_len.resize(n); P.cd_off.resize(n); P.nonce.resize(n); P.circuit.resize(n);
    P.key_x.resize(n * 32); P.key_odd.resize(n); P.sig.resize(n * 96); P.cid.resize(n * 32); P.tok.resize(n * 64);
    BinReader r(txs, (size_t)len);
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        P.rec_off[i] = r.pos;
        if (const uint8_t* b = r.bytes(32, "PointCompressed.0")) memcpy(&P.key_x[32 * i], b, 32);
        P.key_odd[i] = r.boolean("PointCompressed.1") ? 1 : 0;
        P.nonce[i] = r.u32("MpnWithdraw.mpn_withdraw_nonce");
        if (const uint8_t* b = r.bytes(96, "Signature")) memcpy(&P.sig[96 * i], b, 96);
        P.pay_off[i] = r.pos;
        skip_string(r);
        parse_contract_id(r, &P.cid[32 * i]);
        P.circuit[i] = r.u32("withdraw_circuit_id");
        P.cd_off[i] = (uint32_t)(r.pos - P.pay_off[i]);
        if (r.ok && r.pos - P.pay_off[i] > MPN_WD_PAYMENT_MAX) r.fail("ContractWithdraw longer than 65536 bytes");
        r.bytes(32, "calldata");
        skip_l1_pub(r);
        parse_contract_id(r, &P.tok[64 * i]);
        P.amounts[2 * i] = r.u64("Amount");
        parse_contract_id(r, &P.tok[64 * i + 32]);
        P.amounts[2 * i + 1] = r.u64("Amount");
        if (r.ok && r.pos - P.pay_off[i] > MPN_WD_PAYMENT_MAX) r.fail("ContractWithdraw longer than 65536 bytes");
        P.pay_len[i] = (uint32_t)(r.pos - P.pay_off[i]);
        if (!r.ok) r.err = "record " + std::to_string(i) + ": " + r.err;
    }
    if (r.ok) P.rec_off[n] = r.pos;
    if (r.ok && r.pos != len) r.fail("bytes after the last record");
    err = r.err;
    return r.ok;
}
struct DpParsed {
    const uint8_t* txs = nullptr;
    std::vector<uint64_t> rec_off, pay_off, amount;
    std::vector<uint32_t> pay_len, tag_off, src_off, sig_off, circuit;
    std::vector<uint8_t> has_sig, key_x, key_odd, cid, tok;  // cid n x 32: payment.contract_id as a scalar; tok n x 32: amount.token_id
    DpSoA soa() const {
        return {txs, rec_off.data(), pay_off.data(), tag_off.data(), src_off.data(), sig_off.data(), has_sig.data(), key_x.data(), key_odd.data()};
    }
};
inline bool parse_deposits(const uint8_t* txs, uint64_t len, uint64_t n, uint32_t flags, DpParsed& P, std::string& err) {
    if (n > len / 150) {  // the shortest record: 33 + (8 + 4 + 4 + 32 + 40 + 2 x 12 + 4 + 1)
        err = "fewer bytes than " + std::to_string(n) + " MpnDeposit records need";
        return false;
    }
    P.txs = txs;
    P.rec_off.resize(n + 1); P.pay_off.resize(n); P.amount.resize(n);
    P.pay_len.resize(n); P.tag_off.resize(n); P.src_off.resize(n); P.sig_off.resize(n); P.circuit.resize(n);
    P.has_sig.resize(n); P.key_x.resize(n * 32); P.key_odd.resize(n); P.cid.resize(n * 32); P.tok.resize(n * 32);
    BinReader r(txs, (size_t)len);
    uint8_t fee_tok[32];
    const char* too_long = "ContractDeposit longer than 65536 bytes";
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        P.rec_off[i] = r.pos;
        if (const uint8_t* b = r.bytes(32, "PointCompressed.0")) memcpy(&P.key_x[32 * i], b, 32);
        P.key_odd[i] = r.boolean("PointCompressed.1") ? 1 : 0;
        P.pay_off[i] = r.pos;
        skip_string(r);
        if (r.ok && r.pos - P.pay_off[i] > MPN_WD_PAYMENT_MAX) r.fail(too_long);
        parse_contract_id(r, &P.cid[32 * i]);
        P.circuit[i] = r.u32("deposit_circuit_id");
        r.bytes(32, "calldata");
        if (r.u64("ed25519 public key length") != 32) r.fail("ed25519 public key length");
        P.src_off[i] = (uint32_t)(r.pos - P.pay_off[i]);
        r.bytes(32, "ed25519 public key");
        parse_contract_id(r, &P.tok[32 * i]);
        P.amount[i] = r.u64("Amount");
        parse_contract_id(r, fee_tok);
        r.u64("Amount");
        r.u32("nonce");
        P.tag_off[i] = (uint32_t)(r.pos - P.pay_off[i]);
        const uint8_t some = r.u8("Option<Signature> tag");
        if (r.ok && some > 1) r.fail("Option tag");
        P.has_sig[i] = some == 1;
        P.sig_off[i] = 0;
        if (r.ok && some) {
            if (flags & BZK_WORK_SIG_LEN_PREFIXED)
                if (r.u64("ed25519 signature length") != 64) r.fail("ed25519 signature length");
            P.sig_off[i] = (uint32_t)(r.pos - P.pay_off[i]);
            r.bytes(64, "ed25519 signature");
        }
        if (r.ok && r.pos - P.pay_off[i] > MPN_WD_PAYMENT_MAX) r.fail(too_long);
        P.pay_len[i] = (uint32_t)(r.pos - P.pay_off[i]);
        if (!r.ok) r.err = "record " + std::to_string(i) + ": " + r.err;
    }
    if (r.ok) P.rec_off[n] = r.pos;
    if (r.ok && r.pos != len) r.fail("bytes after the last record");
    err = r.err;
    return r.ok;
}

// ---- L1 transactions (src/core/transaction.rs:313-363): structure only ------------------------------------------------------------------
// parse_l1_txs cuts n consecutive bincode(Transaction) / bincode(TransactionAndDelta) records into what the device needs to hash the signed
// form in place (bzk_l1.h L1Rec): where the key, the signature and the Signature tag lie and, for CreateContract { state: Some } /
// UpdateContract { delta: Some }, the byte range of that option.  No hashing and no field arithmetic.  What a record's structure does not
// show stays with the node's deserializer: canonical scalars, valid curve points inside verifying keys, the token-name regex
// (Token::validate), ZkStateModel::is_valid.  That is why the model and the pairs are walked here and not by state.hip's readers, which
// apply the limits of is_valid and of a locator's length on top of bincode's rules.
//
//   Transaction        { src: Option<S::Pub>, nonce u32, data: TransactionData, fee: Money, memo: String, sig: Signature<S> }    :349-357
//   TransactionAndDelta{ tx, state_delta: Option<ZkDeltaPairs> }                                                                 :359-363
//   TransactionData    enum { UpdateStaker 0, Delegate 1, Undelegate 2, AutoDelegate 3, RegularSend 4, CreateContract 5, UpdateContract 6 }
//   Signature<S>       enum { Unsigned = 0, Signed(S::Sig) = 1 }                                                  src/core/address.rs:34-37
//   ContractUpdate     { circuit_id u32, data: ContractUpdateData, next_state: ZkCompressedState, prover, reward: Amount, proof: ZkProof }
//   ContractUpdateData enum { Deposit { Vec<ContractDeposit> } 0, Withdraw { Vec<ContractWithdraw> } 1, FunctionCall { fee } 2, Mint { amount } 3 }
//   ZkContract         { initial_state, state_model, deposit_functions, withdraw_functions: Vec<ZkMultiInputVerifierKey { vk, u8 }>,
//                        functions: Vec<ZkSingleInputVerifierKey { vk }>, token: Option<ZkTokenContract { Token, Vec<Single..> }> }  src/zk/mod.rs:573-644
//   Token              { name, symbol: String, supply: Amount, decimals u8, minter: Option<S::Pub> }                             :254-261
//   ZkDataPairs / ZkDeltaPairs  HashMap<ZkDataLocator(Vec<u64>), ZkScalar / Option<ZkScalar>>                       src/zk/mod.rs:427, 471-474
//
// `V::Pub` of UpdateStaker is schnorrkel's PublicKey; the crate is not vendored [recalled]: under bincode it is a length-prefixed byte string
// of 32, as ed25519_dalek::PublicKey is.
inline bool rd_option_tag(BinReader& r, const char* what) {
    const uint8_t tag = r.u8(what);
    if (r.ok && tag > 1) r.fail(what);
    return r.ok && tag == 1;
}
inline void skip_vrf_pub(BinReader& r) {  // schnorrkel::PublicKey [recalled]
    if (r.u64("vrf public key length") != 32) r.fail("vrf public key length");
    r.bytes(32, "vrf public key");
}
inline void skip_compressed_state(BinReader& r) {
    r.bytes(32, "ZkCompressedState.state_hash");
    r.u64("ZkCompressedState.state_size");
}
inline void skip_state_model(BinReader& r, int depth = 0) {  // enum { Scalar 0, Struct { Vec } 1, List { u8, Box } 2 }
    if (depth > 256) { r.fail("ZkStateModel nested deeper than 256"); return; }  // bounds the recursion, not the reference's rule
    const uint32_t tag = r.u32("ZkStateModel tag");
    if (!r.ok || tag == 0) return;
    if (tag == 1) {
        const uint64_t k = r.len(4, "ZkStateModel::Struct fields");
        for (uint64_t i = 0; i < k && r.ok; ++i) skip_state_model(r, depth + 1);
    } else if (tag == 2) {
        r.u8("ZkStateModel::List log4_size");
        skip_state_model(r, depth + 1);
    } else {
        r.fail("ZkStateModel variant");
    }
}
inline void skip_locator(BinReader& r) {
    const uint64_t k = r.len(8, "ZkDataLocator length");
    r.bytes((size_t)k * 8, "ZkDataLocator");
}
inline void skip_data_pairs(BinReader& r) {
    const uint64_t k = r.len(40, "ZkDataPairs length");
    for (uint64_t i = 0; i < k && r.ok; ++i) {
        skip_locator(r);
        r.bytes(32, "ZkDataPairs value");
    }
}
inline void skip_delta_pairs(BinReader& r) {
    const uint64_t k = r.len(9, "ZkDeltaPairs length");
    for (uint64_t i = 0; i < k && r.ok; ++i) {
        skip_locator(r);
        if (rd_option_tag(r, "ZkDeltaPairs Option tag")) r.bytes(32, "ZkDeltaPairs value");
    }
}
inline void skip_contract_withdraw(BinReader& r) {  // rd_contract_withdraw without its fingerprint: nothing is hashed here
    skip_string(r);
    rd_contract_id(r);
    r.u32("withdraw_circuit_id");
    r.bytes(32, "calldata");
    skip_l1_pub(r);
    rd_money(r);
    rd_money(r);
}
inline void skip_zk_proof(BinReader& r) {  // ZkProof::Groth16(Box<Groth16Proof { a: G1, b: G2, c: G1 }>): u32 0 + 97 + 193 + 97 bytes
    if (r.u32("ZkProof tag") != 0) r.fail("ZkProof variant (only Groth16 = 0 exists outside cfg(test))");
    r.bytes(387, "Groth16Proof");
}
inline void skip_single_vks(BinReader& r, const char* what) {
    const uint64_t k = r.len(882, what);
    for (uint64_t i = 0; i < k && r.ok; ++i) rd_verifier_key(r);
}
inline void skip_multi_vks(BinReader& r, const char* what) {
    const uint64_t k = r.len(883, what);
    for (uint64_t i = 0; i < k && r.ok; ++i) {
        rd_verifier_key(r);
        r.u8("log4_payment_capacity");
    }
}
inline void skip_zk_contract(BinReader& r) {
    skip_compressed_state(r);
    skip_state_model(r);
    skip_multi_vks(r, "ZkContract.deposit_functions");
    skip_multi_vks(r, "ZkContract.withdraw_functions");
    skip_single_vks(r, "ZkContract.functions");
    if (rd_option_tag(r, "Option<ZkTokenContract> tag")) {
        skip_string(r);  // Token.name
        skip_string(r);  // Token.symbol
        r.u64("Token.supply");
        r.u8("Token.decimals");
        if (rd_option_tag(r, "Option<minter> tag")) skip_l1_pub(r);
        skip_single_vks(r, "ZkTokenContract.mint_functions");
    }
}
inline void skip_contract_update(BinReader& r, uint32_t flags) {
    r.u32("ContractUpdate.circuit_id");
    const uint32_t tag = r.u32("ContractUpdateData tag");
    if (!r.ok) return;
    if (tag == 0) {
        const uint64_t k = r.len(117, "ContractUpdateData::Deposit length");
        DepositTx scratch;
        for (uint64_t i = 0; i < k && r.ok; ++i) rd_contract_deposit(r, flags, scratch);
    } else if (tag == 1) {
        const uint64_t k = r.len(112, "ContractUpdateData::Withdraw length");
        for (uint64_t i = 0; i < k && r.ok; ++i) skip_contract_withdraw(r);
    } else if (tag == 2) {
        rd_money(r);
    } else if (tag == 3) {
        r.u64("Mint.amount");
    } else {
        r.fail("ContractUpdateData variant");
    }
    skip_compressed_state(r);
    skip_l1_pub(r);
    r.u64("ContractUpdate.reward");
    skip_zk_proof(r);
}
// ---- rd_contract_update: skip_contract_update's recording twin.  Structure only: where the pieces lie, and whether a payment names the update's
// contract and circuit.  No hashing and no field arithmetic.
inline bool contract_id_is(BinReader& r, const uint8_t cid[32]) {  // reads a ContractId; true where its scalar's bytes are cid's
    uint8_t b[32];
    rd_contract_id(r).to_bytes(b);
    return r.ok && memcmp(b, cid, 32) == 0;
}
inline void rd_update_payment(BinReader& r, uint32_t flags, bool deposit, const uint8_t cid[32], uint32_t circuit_id, size_t rec0, upd::PayRec& p) {
    const size_t p0 = r.pos;
    p.off = (uint32_t)(p0 - rec0);
    p.flags = 0;
    p.tag_off = p.src_off = p.sig_off = p.pad = 0;
    skip_string(r);  // memo
    if (contract_id_is(r, cid)) p.flags |= upd::PAY_CONTRACT;
    if (r.u32("circuit id of the payment") == circuit_id && r.ok) p.flags |= upd::PAY_CIRCUIT;
    p.cd_off = (uint32_t)(r.pos - p0);
    r.bytes(32, "calldata");
    if (r.u64("ed25519 public key length") != 32) r.fail("ed25519 public key length");
    p.src_off = (uint32_t)(r.pos - p0);
    r.bytes(32, "ed25519 public key");  // src of a deposit, dst of a withdrawal
    p.amt_off = (uint32_t)(r.pos - p0);
    rd_money(r);
    p.fee_off = (uint32_t)(r.pos - p0);
    rd_money(r);
    if (deposit) {
        r.u32("nonce");
        p.tag_off = (uint32_t)(r.pos - p0);
        const uint8_t some = r.u8("Option<Signature> tag");
        if (r.ok && some > 1) r.fail("Option tag");
        if (r.ok && some) {
            if (flags & BZK_WORK_SIG_LEN_PREFIXED)
                if (r.u64("ed25519 signature length") != 64) r.fail("ed25519 signature length");
            p.sig_off = (uint32_t)(r.pos - p0);
            r.bytes(64, "ed25519 signature");
            p.flags |= upd::PAY_HAS_SIG;
        }
    }
    p.len = (uint32_t)(r.pos - p0);
}
// u: kind, circuit id, payment range and offsets; its payments are appended to pays with upd = index
inline void rd_contract_update(BinReader& r, uint32_t flags, const uint8_t cid[32], uint32_t index, upd::UpdRec& u, std::vector<upd::PayRec>& pays) {
    const size_t p0 = r.pos;
    u = upd::UpdRec();
    u.at = p0;
    u.slot = upd::NO_SLOT;
    u.circuit_id = r.u32("ContractUpdate.circuit_id");
    u.kind = r.u32("ContractUpdateData tag");
    if (!r.ok) return;
    u.pay0 = (uint32_t)pays.size();
    u.data_off = (uint32_t)(r.pos - p0);
    if (u.kind == upd::DEPOSIT || u.kind == upd::WITHDRAW) {
        const bool deposit = u.kind == upd::DEPOSIT;
        const uint64_t k = r.len(deposit ? 117 : 112, deposit ? "ContractUpdateData::Deposit length" : "ContractUpdateData::Withdraw length");
        for (uint64_t i = 0; i < k && r.ok; ++i) {
            upd::PayRec p;
            p.upd = index;
            p.slot = (uint32_t)i;
            rd_update_payment(r, flags, deposit, cid, u.circuit_id, p0, p);
            if (r.ok) pays.push_back(p);
        }
        u.pay_n = (uint32_t)(pays.size() - u.pay0);
    } else if (u.kind == upd::CALL) {
        rd_money(r);
    } else if (u.kind == upd::MINT) {
        r.u64("Mint.amount");
    } else {
        r.fail("ContractUpdateData variant");
    }
    u.next_off = (uint32_t)(r.pos - p0);
    skip_compressed_state(r);
    u.commit_off = (uint32_t)(r.pos - p0);
    skip_l1_pub(r);
    r.u64("ContractUpdate.reward");
    if (r.u32("ZkProof tag") != 0) r.fail("ZkProof variant (only Groth16 = 0 exists outside cfg(test))");
    u.proof_off = (uint32_t)(r.pos - p0);
    r.bytes(upd::PROOF_BYTES, "Groth16Proof");
    if (r.ok && r.pos - p0 > upd::RECORD_MAX) r.fail("record longer than 1048576 bytes");
}
struct UpdParsed {
    const uint8_t* bytes = nullptr;
    uint64_t len = 0;
    std::vector<upd::UpdRec> rec;   // n
    std::vector<upd::PayRec> pay;   // every payment of the call, in record order
    uint64_t end(uint64_t i) const { return i + 1 < rec.size() ? rec[i + 1].at : len; }  // where record i ends
};
// false with err naming the record when the bytes are not n well-formed ContractUpdate records
inline bool parse_contract_updates(const uint8_t* bytes, uint64_t len, uint64_t n, uint32_t flags, const uint8_t cid[32], UpdParsed& P, std::string& err) {
    if (n > len / 495) {  // the shortest record: 4 + 4 + 8 + 40 + 40 + 8 + 4 + 387
        err = "record " + std::to_string(len / 495) + ": the input ends before it (" + std::to_string(n) + " ContractUpdate records need 495 bytes each)";
        return false;
    }
    P.bytes = bytes;
    P.len = len;
    P.rec.resize(n);
    P.pay.clear();
    BinReader r(bytes, (size_t)len);
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        rd_contract_update(r, flags, cid, (uint32_t)i, P.rec[i], P.pay);
        if (r.ok && P.pay.size() >= ((uint64_t)1 << 31)) r.fail("more than 2^31 payments in one call");
        if (!r.ok) r.err = "record " + std::to_string(i) + ": " + r.err;
    }
    if (r.ok && r.pos != len) {
        r.fail("bytes after the last record");
        if (n) r.err = "record " + std::to_string(n - 1) + ": " + r.err;
    }
    err = r.err;
    return r.ok;
}
// what bzk_l1_tx_updates collects while rd_l1_tx walks an UpdateContract: (transaction, offset in the input, length) of every update of contract cid
struct UpdSpans {
    const uint8_t* cid;
    uint64_t tx = 0;
    std::vector<uint64_t> out;
    // bzk_l1_tx_deltas: per UpdateContract of cid (transaction, offset of the ZkDeltaPairs body, length, source: 0 `delta`, 1 `state_delta`, 2 none)
    std::vector<uint64_t> deltas;
};
// an Option in the middle of the record that the signature leaves out: [cut_a, cut_b) where it is Some, empty otherwise
template <class Skip>
inline void rd_cut_option(BinReader& r, size_t p0, l1::L1Rec& o, const char* what, Skip skip) {
    const size_t at = r.pos;
    if (!rd_option_tag(r, what)) return;
    skip(r);
    if (r.ok) {
        o.cut_a = (uint32_t)(at - p0);
        o.cut_b = (uint32_t)(r.pos - p0);
    }
}
inline void rd_l1_tx(BinReader& r, uint32_t flags, bool and_delta, l1::L1Rec& o, UpdSpans* spans = nullptr) {
    const size_t p0 = r.pos;
    bool upd_listed = false;  // an UpdateContract of spans->cid: where its delta lies
    uint64_t d_off = 0, d_len = 0, d_src = 2;
    o = l1::L1Rec();
    if (rd_option_tag(r, "Option<src> tag")) {
        if (r.u64("ed25519 public key length") != 32) r.fail("ed25519 public key length");
        o.key_off = (uint32_t)(r.pos - p0);
        r.bytes(32, "ed25519 public key");
        o.flags |= l1::HAS_SRC;
    }
    r.u32("nonce");
    const uint32_t tag = r.u32("TransactionData tag");
    if (!r.ok) return;
    switch (tag) {
    case 0:  // UpdateStaker { vrf_pub_key, commission: Ratio }
        skip_vrf_pub(r);
        r.u8("commission");
        break;
    case 1:  // Delegate { amount, to }
    case 2:  // Undelegate { amount, from }
        r.u64("Amount");
        skip_l1_pub(r);
        break;
    case 3:  // AutoDelegate { to, ratio }
        skip_l1_pub(r);
        r.u8("ratio");
        break;
    case 4: {  // RegularSend { entries: Vec<{ dst, amount: Money }> }
        const uint64_t k = r.len(52, "RegularSend entries");
        for (uint64_t i = 0; i < k && r.ok; ++i) {
            skip_l1_pub(r);
            rd_money(r);
        }
        break;
    }
    case 5:  // CreateContract { contract, money, state: Option<ZkDataPairs> }
        skip_zk_contract(r);
        rd_money(r);
        rd_cut_option(r, p0, o, "Option<ZkDataPairs> tag", skip_data_pairs);
        break;
    case 6: {  // UpdateContract { contract_id, updates, delta: Option<ZkDeltaPairs> }
        const bool listed = spans ? contract_id_is(r, spans->cid) : (rd_contract_id(r), false);
        const uint64_t k = r.len(495, "UpdateContract updates");
        for (uint64_t i = 0; i < k && r.ok; ++i) {
            const size_t a = r.pos;
            skip_contract_update(r, flags);
            if (listed && r.ok) spans->out.insert(spans->out.end(), {spans->tx, (uint64_t)a, (uint64_t)(r.pos - a)});
        }
        const size_t at = r.pos;
        rd_cut_option(r, p0, o, "Option<ZkDeltaPairs> tag", skip_delta_pairs);
        upd_listed = listed;
        if (r.ok && r.pos > at + 1) d_off = at + 1, d_len = r.pos - at - 1, d_src = 0;
        break;
    }
    default:
        r.fail("TransactionData variant");
    }
    rd_money(r);     // fee
    skip_string(r);  // memo
    o.sig_tag = (uint32_t)(r.pos - p0);
    o.sig_tagv = r.u32("Signature tag");
    if (r.ok && o.sig_tagv > 1) r.fail("Signature variant");
    if (r.ok && o.sig_tagv == 1) {
        if (flags & BZK_WORK_SIG_LEN_PREFIXED)
            if (r.u64("ed25519 signature length") != 64) r.fail("ed25519 signature length");
        o.sig_off = (uint32_t)(r.pos - p0);
        r.bytes(64, "ed25519 signature");
        o.flags |= l1::SIGNED;
    }
    if (and_delta) {
        const size_t at = r.pos;
        if (rd_option_tag(r, "Option<state_delta> tag")) {
            skip_delta_pairs(r);
            if (r.ok && d_src == 2) d_off = at + 1, d_len = r.pos - at - 1, d_src = 1;
        }
    }
    if (upd_listed && r.ok) spans->deltas.insert(spans->deltas.end(), {spans->tx, d_off, d_len, d_src});
    if (r.ok && r.pos - p0 > l1::RECORD_MAX) r.fail("record longer than 1048576 bytes");
}
struct L1Parsed {
    const uint8_t* txs = nullptr;
    std::vector<uint64_t> rec_off;  // n + 1
    std::vector<l1::L1Rec> rec;     // n
    L1SoA soa() const { return {txs, rec_off.data(), rec.data()}; }
};
// and_delta: the records are TransactionAndDelta.  false with err naming the record when the bytes are not n well-formed records
inline bool parse_l1_txs(const uint8_t* txs, uint64_t len, uint64_t n, bool and_delta, uint32_t flags, L1Parsed& P, std::string& err,
                         UpdSpans* spans = nullptr) {
    if (n > len / 29) {  // the shortest record: 1 + 4 + (4 + 8) + 4 + 8 + 4, and a TransactionAndDelta's tag
        err = "record " + std::to_string(len / 29) + ": the input ends before it (" + std::to_string(n) + " Transaction records need 29 bytes each)";
        return false;
    }
    P.txs = txs;
    P.rec_off.resize(n + 1);
    P.rec.resize(n);
    BinReader r(txs, (size_t)len);
    for (uint64_t i = 0; i < n && r.ok; ++i) {
        P.rec_off[i] = r.pos;
        if (spans) spans->tx = i;
        rd_l1_tx(r, flags, and_delta, P.rec[i], spans);
        if (!r.ok) r.err = "record " + std::to_string(i) + ": " + r.err;
    }
    if (r.ok) P.rec_off[n] = r.pos;
    if (r.ok && r.pos != len) {
        r.fail("bytes after the last record");
        if (n) r.err = "record " + std::to_string(n - 1) + ": " + r.err;
    }
    err = r.err;
    return r.ok;
}

}  // namespace bzk
