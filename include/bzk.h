/* bzk.h - C ABI of the MI355X-native Groth16 hot path for Bazuka's MPN rollup (libbzk.so).
 *
 * This is the drop-in boundary a Rust host binds with `extern "C"`.  Each entry
 * point names the reference interface it replaces; paths are relative to ziesha-network/bazuka.
 *
 * Conventions
 *  - plain pointers and sizes only; the caller owns every buffer; nothing allocated by the library
 *    crosses the boundary except opaque handles (bzk_ctx, bzk_params) released by their destroy call;
 *  - every function returns an int32 status: 0 = BZK_OK, negative = BZK_E_*; no exceptions, no abort;
 *  - one ctx is bound to one GPU and one HIP stream and may be used from one thread at a time;
 *    distinct ctxs are independent (one process per GPU is the intended deployment);
 *  - scalars are 32-byte little-endian limbs.  Default = MONTGOMERY form, i.e. the in-memory
 *    `ZkScalar` / `bls12_381::Scalar` (src/zk/mod.rs:202-206; transmute-compatible per
 *    src/zk/groth16/mod.rs:7-17).  BZK_F_CANONICAL selects canonical integers (test drivers);
 *  - Fp elements are 48-byte little-endian Montgomery limbs (R = 2^384), as `Fp([u64;6])` in
 *    src/zk/groth16/mod.rs:19-20.  G1 affine = x|y (96 B, "raw", never the identity) or x|y|inf
 *    (97 B, "packed", as `(Fp, Fp, bool)` at :33-38).  G2 = x.c0|x.c1|y.c0|y.c1 (192 B raw) or +inf
 *    (193 B packed).  A Groth16 proof is a|b|c = 97+193+97 = 387 B (= bincode of `Groth16Proof`);
 *  - `*_dev` variants take DEVICE pointers (HBM-resident data; what bench.py times).  The plain
 *    variants take HOST pointers and stage through PCIe.
 *  - There is NO CPU fallback: without a usable gfx950 device bzk_ctx_create fails with
 *    BZK_E_DEVICE and nothing else can be called.
 */
#ifndef BZK_H
#define BZK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BZK_OK 0
#define BZK_E_ARG (-1)      /* bad argument (null pointer, size out of range, arity > 16 ...) */
#define BZK_E_ALLOC (-2)    /* device or host allocation failed */
#define BZK_E_DEVICE (-3)   /* HIP runtime / kernel launch error, or no gfx950 device */
#define BZK_E_UNSAT (-4)    /* witness does not satisfy the constraint system */
#define BZK_E_INTERNAL (-5) /* invariant violated (bug) */

#define BZK_F_CANONICAL 1u  /* scalars are canonical integers instead of Montgomery limbs */
#define BZK_F_DEDUP 2u      /* MSM entries: the scalar vector repeats itself (a Groth16 witness): bases of equal scalars
                             * are summed once before the bucket phase, zero scalars dropped.  Same result. */
#define BZK_F_THROUGHPUT 4u /* MSM entries: this call overlaps other device work (the five MSMs of a proof): prefer the
                             * forms that do less arithmetic over those with the shortest dependency chain (two-level
                             * bucket reduction).  Same result. */

typedef struct bzk_ctx bzk_ctx;

/* ---- context ------------------------------------------------------------------------------- */
/* device_id: HIP ordinal.  stream: a hipStream_t the caller owns (e.g. torch's current stream), or
 * NULL to let the ctx create its own non-blocking stream. */
int32_t bzk_ctx_create(int32_t device_id, void* stream, bzk_ctx** out);
void bzk_ctx_destroy(bzk_ctx* ctx);
int32_t bzk_sync(bzk_ctx* ctx); /* wait for the ctx stream */
const char* bzk_strerror(int32_t status);
const char* bzk_last_error(bzk_ctx* ctx); /* detail of the last BZK_E_DEVICE on this ctx */
/* Which of the reference's errors the last BZK_E_ARG of a bzk_state_* call on this ctx stands for, so that a Rust host can return
 * `StateManagerError::{LocatorError(InvalidLocator), NonScalarLocatorError, NonTreeLocatorError}` (src/zk/state/mod.rs:12-27,
 * src/zk/mod.rs:348-351) instead of parsing bzk_last_error; 0 after a state call that was not refused.  OTHER = malformed input the
 * reference cannot express (bad bincode, locator offsets out of order, counts beyond the ABI's limits). */
#define BZK_REFUSE_NONE 0
#define BZK_REFUSE_INVALID_LOCATOR 1     /* names nothing in the model, index beyond a list / struct, points below a scalar */
#define BZK_REFUSE_NON_SCALAR_LOCATOR 2  /* ends above a scalar where a scalar is written */
#define BZK_REFUSE_NON_TREE_LOCATOR 3    /* `prove` on something that is not a list */
#define BZK_REFUSE_DUPLICATE_LOCATOR 4   /* the same locator twice in one delta (a HashMap cannot hold that) */
#define BZK_REFUSE_NON_CANONICAL_VALUE 5 /* 32 bytes that are not the Montgomery limbs of a residue (a ZkScalar cannot hold that) */
#define BZK_REFUSE_OTHER 6
int32_t bzk_last_refusal(bzk_ctx* ctx);
uint32_t bzk_abi_version(void);

/* device-memory plumbing for hosts that want to keep inputs resident without a tensor library */
int32_t bzk_dev_alloc(bzk_ctx* ctx, uint64_t bytes, void** dptr);
int32_t bzk_dev_free(bzk_ctx* ctx, void* dptr);
/* The call workspace of a ctx is grow-only (one slab, re-used by every call: no allocation on the hot path).  After a one-off large
 * call - a 2^26-point MSM leaves ~24 GB behind - bzk_ctx_trim waits for the stream and hands the slab back to the device; the next
 * call allocates what it needs.  *released (may be NULL) = bytes freed.  (A context whose stand-alone G1 MSM calls run as two window ranges in
 * flight - 2^18 <= n < 2^20 points, DESIGN 3.2d - owns a child context with a workspace of its own and a buffer for converted raw bases: both are
 * released as well.) */
int32_t bzk_ctx_trim(bzk_ctx* ctx, uint64_t* released);
int32_t bzk_h2d(bzk_ctx* ctx, void* dst_dev, const void* src_host, uint64_t bytes);
int32_t bzk_d2h(bzk_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes);

/* per-kernel timing with HIP events on the ctx stream (used by bench.py for `roofline.achieved`) */
int32_t bzk_prof_enable(bzk_ctx* ctx, int32_t on);
/* restrict the event pairs to launches whose label contains `substr` (NULL: every launch).  Timing every launch costs two event
 * creations per kernel (~0.25 ms per 2^20-point MSM with its ~25 launches); bench.py times only the dominant kernel inside its
 * timed region */
int32_t bzk_prof_filter(bzk_ctx* ctx, const char* substr);
int32_t bzk_prof_reset(bzk_ctx* ctx);
/* sums over launches whose kernel label == name; synchronises the stream */
int32_t bzk_prof_query(bzk_ctx* ctx, const char* name, uint64_t* launches, double* total_ms);
/* writes up to cap bytes of "name launches total_ms\n" lines */
int32_t bzk_prof_dump(bzk_ctx* ctx, char* buf, uint64_t cap);

/* ---- K1: batched Poseidon --------------------------------------------------------------------
 * Replaces `ZkHasher::hash` = `PoseidonHasher::hash` -> `poseidon::poseidon`
 * (src/zk/mod.rs:152-155, 496-511; src/zk/poseidon/mod.rs:24-84) for n independent inputs.
 * in: n*arity scalars (hash i uses in[i*arity .. (i+1)*arity)), out: n scalars.  1 <= arity <= 16
 * (MAX_ARITY, src/zk/poseidon/params/mod.rs:25); other arities -> BZK_E_ARG where the reference
 * panics.  Always Montgomery form. */
int32_t bzk_poseidon_batch(bzk_ctx* ctx, const uint8_t* in, uint32_t arity, uint64_t n, uint8_t* out);
int32_t bzk_poseidon_batch_dev(bzk_ctx* ctx, const void* in_dev, uint32_t arity, uint64_t n, void* out_dev);

/* ---- batched EdDSA verification -------------------------------------------------------------------
 * JubJub::<ZkHasher>::verify (src/crypto/jubjub/mod.rs:151-167) for n independent (key, message, signature) triples.
 * pub_xy: n x 64, msg: n x 32, sig: n x 96 (r.x | r.y | s) - the layouts of bzk_host_jubjub_verify.  ok: n bytes, 1 / 0.
 * n = 0 is a no-op.  A 32-byte field that is not the limbs of a residue gives verdict 0 for its entry, not an error.  The host
 * form stages through the context's workspace and synchronises; the _dev form enqueues on the context's stream. */
int32_t bzk_jubjub_verify_batch(bzk_ctx* ctx, const uint8_t* pub_xy, const uint8_t* msg, const uint8_t* sig, uint64_t n, uint8_t* ok);
int32_t bzk_jubjub_verify_batch_dev(bzk_ctx* ctx, const void* pub_xy_dev, const void* msg_dev, const void* sig_dev, uint64_t n, void* ok_dev);

/* ---- batched key decompression ----------------------------------------------------------------------
 * PointCompressed::decompress (src/crypto/jubjub/curve.rs:78-88) for n keys, one lane each: y = sqrt((1 + x^2) / (1 - d x^2)) with the
 * parity of its canonical integer equal to odd.  x: n x 32 (Montgomery), odd: n bytes (0 / non-zero), xy_out: n x 64 (x | y), ok: n bytes.
 * ok = 0 and xy_out = zeros where the reference panics (the radicand has no square root) or x is not the limbs of a residue; y = 0
 * (x^2 = -1) is accepted for either parity.  n = 0 is a no-op.  The host form stages through the context's workspace and synchronises;
 * the _dev form enqueues on the context's stream. */
int32_t bzk_jubjub_decompress_batch(bzk_ctx* ctx, const uint8_t* x, const uint8_t* odd, uint64_t n, uint8_t* xy_out, uint8_t* ok);
int32_t bzk_jubjub_decompress_batch_dev(bzk_ctx* ctx, const void* x_dev, const void* odd_dev, uint64_t n, void* xy_out_dev, void* ok_dev);
/* JubJub::verify as the reference calls it, on a compressed PublicKey: decompress, then bzk_jubjub_verify_batch.  ok = 0 where the key
 * does not decompress.  The _dev form keeps the decompressed keys in the context's workspace (65 bytes per key). */
int32_t bzk_jubjub_verify_batch_compressed(bzk_ctx* ctx, const uint8_t* pk_x, const uint8_t* pk_odd, const uint8_t* msg, const uint8_t* sig,
                                           uint64_t n, uint8_t* ok);
int32_t bzk_jubjub_verify_batch_compressed_dev(bzk_ctx* ctx, const void* pk_x_dev, const void* pk_odd_dev, const void* msg_dev,
                                               const void* sig_dev, uint64_t n, void* ok_dev);
/* MpnTransaction::verify_signature (src/zk/mod.rs:610-627) for n transactions given as n consecutive bincode(MpnTransaction) (nonce u32,
 * two PointCompressed, two Money, Signature: 190 - 254 bytes each, len bytes in all).  ok: n bytes.  hash_out (n x 32, may be NULL) =
 * tx.hash(), zeros where dst does not decompress.  BZK_E_ARG with bzk_mpn_work_last_error() set when the bytes are not n well-formed
 * records; a record whose keys do not decompress, or whose scalars are not residues' limbs, is a verdict 0 (hash zeros), not an error.
 * The host only parses: both keys are decompressed, the integers brought into Montgomery form, the message hashed and the signature
 * checked on the device, in rounds of 2^16 transactions; synchronises.  ctx = NULL: the same on host threads (bzk_host_default_threads). */
int32_t bzk_mpn_tx_verify_batch(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok, uint8_t* hash_out);

/* ---- batched EdDSA key derivation and signing ------------------------------------------------------------
 * JubJub::generate_keys and JubJub::sign (src/crypto/jubjub/mod.rs:112-150) for n independent rows, one lane each.  Signing is deterministic:
 * r = Poseidon(randomness, msg), R = r BASE, h = Poseidon(R.x, R.y, pk.x, pk.y, msg), s = (r + h a) mod ORDER, so the bytes equal
 * bzk_host_jubjub_sign's and bzk_host_jubjub_keys'.
 * keys: seed i = seeds[off[i] .. off[i+1]) (off: n + 1 non-decreasing entries from 0, as bzk_sha3_256_batch takes its messages), keys_out
 * n x 128 (pub.x | pub.y | randomness | scalar).
 * sign: keys n x 128 in that layout, msg n x 32, sig_out n x 96 (r.x | r.y | s), ok n bytes.  pub is taken as given (not checked against
 * scalar BASE).  A key field or message that is not the limbs of a residue gives ok = 0 and 96 zero bytes for its row, not an error
 * (bzk_host_jubjub_sign does not validate).  n = 0 is a no-op.
 * The host forms stage through the context's workspace in rounds of 2^16 rows, synchronise, and overwrite the workspace regions that held
 * key bytes before they return; the _dev forms enqueue on the context's stream, trust off and leave the caller's buffers alone.  ctx = NULL
 * (host forms): the same per-lane code on host threads (bzk_host_default_threads).  The fixed-base walk indexes a table by nibbles of the
 * secret nonce: fixed-flow, not address-independent - a throughput signer, not a hardened one. */
int32_t bzk_jubjub_keys_batch(bzk_ctx* ctx, const uint8_t* seeds, const uint64_t* off, uint64_t n, uint8_t* keys_out);
int32_t bzk_jubjub_keys_batch_dev(bzk_ctx* ctx, const void* seeds_dev, const void* off_dev, uint64_t n, void* keys_out_dev);
int32_t bzk_jubjub_sign_batch(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* msg, uint64_t n, uint8_t* sig_out, uint8_t* ok);
int32_t bzk_jubjub_sign_batch_dev(bzk_ctx* ctx, const void* keys_dev, const void* msg_dev, uint64_t n, void* sig_out_dev, void* ok_dev);
/* TxBuilder::create_mpn_transaction's signing step for n transactions given as n consecutive bincode(MpnTransaction) (bzk_mpn_tx_verify_batch's
 * input; the 96 signature bytes of the input are ignored) and n keys (n x 128).  The host only parses; per record the device decompresses
 * dst, computes tx.hash(), checks that src is the compression of the key's pub, and signs.  txs_out (len bytes) = the input with each signed
 * record's signature replaced; ok[i] = 0 and record i copied unchanged where dst does not decompress, a token id is not a residue's limbs,
 * src does not match the key or a key field is not a residue's limbs.  hash_out (n x 32, may be NULL) = tx.hash(), zeros where it could not
 * be computed.  BZK_E_ARG with bzk_mpn_work_last_error() set when the bytes are not n well-formed records.  Rounds of 2^16 records;
 * synchronises; the staged key bytes are overwritten.  ctx = NULL: the same on host threads. */
int32_t bzk_mpn_txs_sign(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* txs_out, uint8_t* ok,
                         uint8_t* hash_out);
/* TxBuilder::withdraw_mpn (src/wallet/tx_builder.rs:376-425) for n withdrawals given as n consecutive bincode(MpnWithdraw)
 * (bzk_mpn_withdraw_verify_batch's input; the 96 mpn_sig bytes and the 32 payment.calldata bytes of the input are ignored whatever they hold)
 * and n keys (n x 128, the layout of bzk_jubjub_sign_batch).  The host only parses; per record the device computes payment.fingerprint()
 * (SHA3-256 with the calldata read as zeros, then ZkScalar::new), checks that mpn_address is the compression of the key's pub, signs
 * Poseidon(fingerprint, nonce) and computes calldata = Poseidon(pub.x, pub.y, nonce, sig.r.x, sig.r.y, sig.s).  txs_out (len bytes, may be
 * txs) = the input with each signed record's mpn_sig and payment.calldata replaced, both as bzk_mpn_withdraw_verify_batch reads them (32-byte
 * Montgomery limbs); a record's length never changes.  ok[i] = 1 where record i was signed; ok[i] = 0 and record i copied unchanged where a
 * key field is not the limbs of a residue or mpn_address does not match the key, not an error.  fingerprint_out (n x 32, may be NULL) =
 * payment.fingerprint() for every record, signed or not: the bytes bzk_mpn_withdraw_verify_batch returns.  BZK_E_ARG with
 * bzk_mpn_work_last_error() naming the record when the bytes are not n well-formed records, nothing written; a payment longer than 65 536
 * bytes counts as malformed, as on the verify side.  n = 0 is a no-op.  Rounds end at 2^16 records or 64 MiB of payment bytes, whichever
 * comes first; synchronises; the workspace region that held key bytes is overwritten before the call returns, on the error paths too.
 * ctx = NULL: the same per-lane code on host threads (bzk_host_default_threads).  The fixed-base walk indexes a table by nibbles of the secret
 * nonce: fixed-flow, not address-independent - a throughput signer, not a hardened one. */
int32_t bzk_mpn_withdraws_sign(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* txs_out, uint8_t* ok,
                               uint8_t* fingerprint_out);

/* ---- batched SHA3-256 and hash_to_scalar -----------------------------------------------------------------
 * n messages: message i = data[off[i] .. off[i+1]), off has n + 1 entries, off[0] = 0, non-decreasing.  One lane per message, which loops
 * over as many 136-byte blocks as its own length needs (FIPS 202: rate 136, suffix 0x06, final 0x80).
 * digest_out (n x 32, may be NULL) = SHA3-256; scalar_out (n x 32, may be NULL) = hash_to_scalar (src/zk/mod.rs:218-220), i.e.
 * ZkScalar::new of the digest read as a little-endian integer, Montgomery.  At least one of the two outputs must be given.  n = 0 is a
 * no-op.  The host form checks off, stages through the context's workspace (in rounds of 2^20 messages or 64 MiB) and synchronises; the
 * _dev form enqueues on the context's stream and trusts off (digest_out_dev 4-byte, scalar_out_dev 16-byte aligned). */
int32_t bzk_sha3_256_batch(bzk_ctx* ctx, const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* digest_out, uint8_t* scalar_out);
int32_t bzk_sha3_256_batch_dev(bzk_ctx* ctx, const void* data_dev, const void* off_dev, uint64_t n, void* digest_out_dev, void* scalar_out_dev);
/* MpnWithdraw's two checks for n withdrawals given as n consecutive bincode(MpnWithdraw) (PointCompressed, u32 nonce, Signature,
 * ContractWithdraw: 245 bytes and up, len bytes in all).  ok[i]: bit 0 = MpnWithdraw::verify_signature (src/core/transaction.rs:183-189),
 * bit 1 = verify_calldata (:177-182; the payment's 32 calldata bytes are compared as bytes with the limbs of H6's output).
 * fingerprint_out (n x 32, may be NULL) = payment.fingerprint() (:204-211): SHA3-256 of the payment with its calldata read as zeros, then
 * ZkScalar::new.  BZK_E_ARG with bzk_mpn_work_last_error() naming the record when the bytes are not n well-formed records, nothing written;
 * a payment longer than 65 536 bytes is refused as malformed too (its memo is unbounded on the wire), on both paths.  A key that does not
 * decompress, or key / signature scalars that are not residues' limbs, give ok = 0 for that record, not an error.  The host only parses:
 * fingerprint, key decompression, both Poseidon hashes and the signature check run on the device, in rounds that end at 2^16 records or
 * 64 MiB of payment bytes, whichever comes first; synchronises.  ctx = NULL: the same on host threads (bzk_host_default_threads). */
int32_t bzk_mpn_withdraw_verify_batch(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok, uint8_t* fingerprint_out);

/* ---- batched SHA-512 and Ed25519; wire-form deposits ----------------------------------------------------------
 * SHA-512 (FIPS 180-4) of n messages laid out as for bzk_sha3_256_batch (off: n + 1 non-decreasing entries from 0); digest_out n x 64.  One
 * lane per message.  n = 0 is a no-op; the host form checks off, stages through the workspace (rounds of 2^20 messages or 64 MiB) and
 * synchronises; the _dev form enqueues on the context's stream and trusts off (digest_out_dev 4-byte aligned).  ctx = NULL (host form): the
 * same per-lane code on host threads (bzk_host_default_threads). */
int32_t bzk_sha512_batch(bzk_ctx* ctx, const uint8_t* data, const uint64_t* off, uint64_t n, uint8_t* digest_out);
int32_t bzk_sha512_batch_dev(bzk_ctx* ctx, const void* data_dev, const void* off_dev, uint64_t n, void* digest_out_dev);
/* Ed25519 as the node checks it (`ed25519-dalek = "1"` PublicKey::verify, src/crypto/ed25519.rs:81-83), one lane per signature: pk n x 32,
 * sig n x 64 (R | s), messages as above; ok[i] = 1 / 0.  Cofactorless: encode([s]B - [k]A) == R as bytes, k = SHA-512(R | A | M) mod l; no
 * small-order rejection; s >= l gives 0; A's y is taken mod p without a canonicity check and x = 0 with the sign bit set is accepted; a key
 * that does not decode gives 0, not an error.  The L1 signature of every transaction of a block (src/blockchain/ops/apply_block.rs:88) is this
 * check too.  Conventions as bzk_sha512_batch. */
int32_t bzk_ed25519_verify_batch(bzk_ctx* ctx, const uint8_t* pk, const uint8_t* msg, const uint64_t* off, const uint8_t* sig, uint64_t n,
                                 uint8_t* ok);
int32_t bzk_ed25519_verify_batch_dev(bzk_ctx* ctx, const void* pk_dev, const void* msg_dev, const void* off_dev, const void* sig_dev, uint64_t n,
                                     void* ok_dev);
/* MpnDeposit's checks for n deposits given as n consecutive bincode(MpnDeposit) (PointCompressed, ContractDeposit: 150 bytes and up, len bytes
 * in all).  ok[i]: bit 0 = payment.verify_signature() (src/core/transaction.rs:192-202: Ed25519 by payment.src over the payment's bytes up to
 * the Option<Signature> tag followed by a None tag; sig: None gives 0), bit 1 = mpn_address decompresses (the reference's builder panics
 * where it does not).  addr_xy_out (n x 64, may be NULL) = the decompressed address, zeros where there is none.  BZK_E_ARG with
 * bzk_mpn_work_last_error() naming the record when the bytes are not n well-formed records or a payment is longer than 65 536 bytes; nothing
 * is written then.  The host only parses; rounds end at 2^16 records or 64 MiB of payment bytes; synchronises.  ctx = NULL: the same per-lane
 * code on host threads.  The signature inside the payment is read as the 64-tuple of ed25519 >= 1.3 unless bzk_mpn_set_wire_flags says
 * otherwise. */
int32_t bzk_mpn_deposit_verify_batch(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok, uint8_t* addr_xy_out);
/* process-wide: how wire-form records spell what the work codec takes a flag for (BZK_WORK_SIG_LEN_PREFIXED below, or 0).  Read by
 * bzk_mpn_deposit_verify_batch and bzk_mpn_push_deposits; pass the same flags to bzk_mpn_work_decode for works made from such deposits. */
int32_t bzk_mpn_set_wire_flags(uint32_t flags);

/* ---- wire-form L1 transactions: signature, hash and block root -------------------------------------------------
 * The fourth arm of GeneralTransaction::verify_signature (src/core/mod.rs:163-170) and the cryptographic part of apply_block's body checks.
 * The signed bytes of a Transaction are bincode(tx.sig_state_excluded()) (src/core/transaction.rs:369-397): the record with Signature::Unsigned
 * for its signature and, for CreateContract { state } / UpdateContract { delta }, None for that option.  The host parses the records' structure
 * only (all seven TransactionData variants) and the device hashes that form in place from the uploaded record, as a list of ranges and zero runs.
 * Canonical scalars, valid curve points inside verifying keys and the token-name rules stay with the node's deserializer; nonce, balance and fee
 * rules with its state machine. */
#define BZK_L1_FORM_TX            0   /* n consecutive bincode(Transaction): a block body's elements        */
#define BZK_L1_FORM_TX_AND_DELTA  1   /* n consecutive bincode(TransactionAndDelta): what the mempool gets  */
/* Transaction::verify_signature (transaction.rs:386-397) and Transaction::hash (:383-385).  ok[i] = 1 / 0 (src None: 1; Unsigned: 0);
 * hash_out n x 32, may be NULL.  ctx = NULL: the same per-lane code on host threads.  Ed25519 semantics are bzk_ed25519_verify_batch's.
 * BZK_E_ARG with bzk_mpn_work_last_error() naming the record when the bytes are not n well-formed records (truncation, trailing bytes, an enum
 * or Option tag out of range, a length past the record, a key / signature length other than 32 / 64) or a record is longer than 2^20 bytes
 * (max_block_size, src/config/blockchain.rs:337); nothing is written then.  Signatures are read as bzk_mpn_set_wire_flags says.  n = 0 is a
 * no-op.  One lane per record; rounds end at 2^16 records or 64 MiB of record bytes; synchronises. */
int32_t bzk_l1_tx_verify_batch(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, uint64_t n, uint32_t form, uint8_t* ok, uint8_t* hash_out);
/* MerkleTree::<Sha3Hasher>::new (src/crypto/merkle.rs) for m trees: tree j has count[j] leaves of 32 bytes, consecutive in leaves.  roots_out
 * m x 32 (no leaves: 32 zero bytes; one leaf: the leaf); nodes_out (may be NULL) receives each tree's whole node array in the reference's heap
 * order (MerkleTree.data), tree after tree (max(1, 2 count[j] - 1) nodes each).  One launch per level covers all trees.  m = 0 is a no-op;
 * ctx = NULL (host form): the same per-lane code on host threads.  The _dev form takes device pointers (n_leaves = the sum of count) and
 * works on the context's stream; the levels are laid out on the host, so it reads count_dev back (m x 8 bytes) first and synchronises. */
int32_t bzk_sha3_merkle_roots(bzk_ctx* ctx, const uint8_t* leaves, const uint64_t* count, uint64_t m, uint8_t* roots_out, uint8_t* nodes_out);
int32_t bzk_sha3_merkle_roots_dev(bzk_ctx* ctx, const void* leaves_dev, const void* count_dev, uint64_t m, uint64_t n_leaves, void* roots_out_dev,
                                  void* nodes_out_dev);
/* The body checks of apply_block (src/blockchain/ops/apply_block.rs:47 and :88) for m blocks at once: txs = all bodies' bincode(Transaction)
 * back to back, count[j] per block.  sig_ok_out[j] = every transaction of block j verifies (an empty body: 1); root_out[j] = block j's
 * merkle_tree().root() (src/core/blocks.rs:17-19), to be compared with header.block_root by the caller; tx_ok_out (n bytes) and hash_out
 * (n x 32) may be NULL.  Hashes and trees stay on the device between the two steps.  Refusals as bzk_l1_tx_verify_batch; ctx = NULL as there. */
int32_t bzk_block_bodies_check(bzk_ctx* ctx, const uint8_t* txs, uint64_t len, const uint64_t* count, uint64_t m, uint8_t* sig_ok_out,
                               uint8_t* root_out, uint8_t* tx_ok_out, uint8_t* hash_out);

/* ---- batched Ed25519 key derivation and signing; the producers of deposits and L1 transactions -----------------
 * Ed25519::<Sha3_256>::generate_keys and Ed25519::sign (src/crypto/ed25519.rs:70-80 over `ed25519-dalek = "1"`) for n independent rows, one
 * lane each.  Signing is RFC 8032 5.1.6 and deterministic: h = SHA-512(secret), a = the clamped low half, r = SHA-512(h[32 .. 64) | M) mod l,
 * R = encode([r]B), k = SHA-512(R | A | M) mod l, s = (k a + r) mod l, so every route gives the bytes of bzk_host_ed25519_sign, of dalek and
 * of OpenSSL.
 * keys: seed i = seeds[off[i] .. off[i+1]) (off: n + 1 non-decreasing entries from 0, as bzk_sha512_batch takes its messages);
 * secret = SHA3-256(seed) with bit 255 cleared; keys_out n x 64 (secret | public, the layout of Keypair::to_bytes()).
 * sign: keys n x 64 in that layout, message i = msg[off[i] .. off[i+1]), sig_out n x 64 (R | s).  The public half is taken as given, as
 * dalek's ExpandedSecretKey::sign(message, &public) takes it.  Every key is valid, so there is no ok output.  n = 0 is a no-op.
 * The host forms check off, stage through the context's workspace in rounds that end at 2^16 rows or 64 MiB, synchronise, and overwrite the
 * workspace regions that held staged keys, seeds, expanded scalars and prefixes before they return; the _dev forms enqueue on the context's
 * stream, trust off and leave the caller's buffers alone (the signer's own 64 bytes per row of workspace are overwritten behind the launch).
 * ctx = NULL (host forms): the same per-lane code on host threads (bzk_host_default_threads).  The fixed-base walk indexes a table by
 * nibbles of the secret nonce (of the secret scalar for keys): fixed-flow, not address-independent - a throughput signer, not a hardened one. */
int32_t bzk_ed25519_keys_batch(bzk_ctx* ctx, const uint8_t* seeds, const uint64_t* off, uint64_t n, uint8_t* keys_out);
int32_t bzk_ed25519_keys_batch_dev(bzk_ctx* ctx, const void* seeds_dev, const void* off_dev, uint64_t n, void* keys_out_dev);
int32_t bzk_ed25519_sign_batch(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* msg, const uint64_t* off, uint64_t n, uint8_t* sig_out);
int32_t bzk_ed25519_sign_batch_dev(bzk_ctx* ctx, const void* keys_dev, const void* msg_dev, const void* off_dev, uint64_t n, void* sig_out_dev);
/* TxBuilder::sign_deposit (src/wallet/tx_builder.rs:63-66) for n deposits given as n consecutive bincode(MpnDeposit)
 * (bzk_mpn_deposit_verify_batch's input; payment.sig may be None or Some, a Some's bytes are ignored) and n keys (n x 64).  The signed bytes
 * are the payment up to the Option tag followed by a None tag, hashed in place from the uploaded record.  sig_out n x 64; ok[i] = 1 where
 * payment.src equals the key's public half, else ok[i] = 0, a zero sig_out row and the record copied through unchanged.  txs_out (may be
 * NULL: only sig_out and ok are written) receives the records with Some(sig), spelled as bzk_mpn_set_wire_flags says; *out_len is always set
 * to the length they need; where cap is smaller, BZK_E_ARG and nothing else written.  Refusals of malformed input are
 * bzk_mpn_deposit_verify_batch's, naming the record.  Rounds end at 2^16 records or 64 MiB; synchronises; staged keys and their expansions
 * are overwritten.  ctx = NULL: the same per-lane code on host threads. */
int32_t bzk_mpn_deposits_sign(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* sig_out, uint8_t* ok,
                              uint8_t* txs_out, uint64_t cap, uint64_t* out_len);
/* TxBuilder::sign_tx (src/wallet/tx_builder.rs:67-70) for n records of either BZK_L1_FORM_* form and any TransactionData variant; the
 * signature may be Unsigned or Signed (ignored).  The signed form is bzk_l1_tx_verify_batch's (the state / delta cut and Signature::Unsigned),
 * hashed in place.  ok[i] = 0, a zero sig_out row and the record copied unchanged where src is None or differs from the key's public half.
 * hash_out (n x 32, may be NULL) = Transaction::hash of every record.  txs_out, cap, out_len, rounds, hygiene and ctx = NULL as
 * bzk_mpn_deposits_sign; the records come back with Signature::Signed(sig).  Refusals are bzk_l1_tx_verify_batch's. */
int32_t bzk_l1_txs_sign(bzk_ctx* ctx, const uint8_t* keys, const uint8_t* txs, uint64_t len, uint64_t n, uint32_t form, uint8_t* sig_out, uint8_t* ok,
                        uint8_t* hash_out, uint8_t* txs_out, uint64_t cap, uint64_t* out_len);

/* ---- wire-form ContractUpdates: commitment, aux data, deposit signatures and proof -------------------------------
 * What `update_contract` (src/blockchain/ops/apply_tx/update_contract/mod.rs:28-116) computes and verifies per ContractUpdate before and when
 * it calls zk::check_proof, for the updates of m consecutive UpdateContract transactions of ONE contract: the commitment
 * ZkScalar::new(sha3(bincode((prover, reward)))), aux_data.state_hash (the root of the payments' list for Deposit / Withdraw, deposit.rs:16-55 and
 * withdraw.rs:16-72, with every withdrawal's fingerprint; H2(token, fee) for FunctionCall, function_call.rs:28-44), every deposit's Ed25519
 * signature (apply_deposit.rs:8) and the Groth16 proof over (commit, height, state, aux, next_state).  The host parses the records' structure
 * only; hashing, field arithmetic, signatures and pairings run on the device.  Balances, nonces and fees, Mint, and the delta / state-root check
 * after the updates stay with the node. */
typedef struct { const uint8_t* vk; uint64_t vk_len; uint8_t log4_payment_capacity; } bzk_contract_fn;   /* bincode(Groth16VerifyingKey) */
typedef struct {
    uint8_t contract_id[32];                    /* the scalar the circuits use for ContractId (Null 0, Ziesha 1, Custom its scalar): Montgomery limbs */
    const bzk_contract_fn* deposit_fns;  uint32_t n_deposit_fns;    /* ZkContract.deposit_functions  */
    const bzk_contract_fn* withdraw_fns; uint32_t n_withdraw_fns;   /* ZkContract.withdraw_functions */
    const bzk_contract_fn* fns;          uint32_t n_fns;            /* ZkContract.functions; capacity ignored */
} bzk_contract_desc;
#define BZK_UPD_PROOF 1u        /* zk::check_proof(circuit, commit, height, state, aux, next_state, proof) */
#define BZK_UPD_SIGS  2u        /* every deposit's verify_signature (apply_deposit.rs:8); 1 for the other kinds */
#define BZK_UPD_ROUTE 4u        /* circuit_id names a function of its kind; every payment carries this contract_id and this circuit id
                                   (DepositWithdrawPassedToWrongFunction); payments <= 4^capacity (batch_set's locator rule) */
#define BZK_UPD_UNSUPPORTED 128u   /* 0x80.  ContractUpdateData::Mint: left to the node; the other bits are 0 */
/* updates = n = sum of count bincode(ContractUpdate) records back to back; count[j] of them belong to transaction j.  Every update of
 * transaction j is checked at height height0 + j (update_contract reads prev_account.height once per transaction).  The first update of the call
 * is checked against state0, every later one against the next_state.state_hash that the update BEFORE it claims - whatever that update's own
 * verdict is.  The chain is optimistic: ok[i] says "valid given its predecessor's claim", and the first update with (ok[i] & 7) != 7 is where
 * the sequence breaks; nothing after it may be applied.
 * ok[i]: the BZK_UPD_* bits.  With ROUTE clear the proof is not looked at and PROOF is 0.  A key the single verifier refuses (n_ic != 6, a point
 * off its curve) gives PROOF 0 for all of its updates, as bzk_groth16_verify_batch does; a state0 or next_state.state_hash whose limbs are >= r
 * gives PROOF 0, not an error.  aux_out (n x 32, may be NULL): aux_data.state_hash, zeros where ROUTE fails or for a Mint; commit_out (n x 32,
 * may be NULL): the commitments.  BZK_E_ARG with bzk_mpn_work_last_error() naming the record when the bytes are not n well-formed records, a
 * record is longer than 2^20 bytes, a log4_payment_capacity is above 8, a key is shorter than 878 bytes, or a pointer is NULL with n > 0;
 * nothing is written then.  n = 0 is a no-op.  Signatures inside deposits are read as bzk_mpn_set_wire_flags says.  ctx = NULL: the same
 * per-lane functions on host threads.  Payments are staged in rounds that end at an update boundary before 2^16 payments or 64 MiB of record
 * bytes; the proofs of each (kind, circuit_id) run as one batch of the verifier, the batches one after another.  Synchronises.
 * Memory: the five inputs and the proof of every routed update (547 bytes) and 70 bytes of aux, commitment, bits and slot per update stay on the device
 * for the whole call, beside one round's records (at most 64 MiB + one record) and the verifier's slab (at most 2^16 proofs): the workspace grows
 * by about 0.62 GB per million updates.  There is no limit on n but the device's memory (BZK_E_ALLOC beyond it); a caller syncing more than a
 * few million updates of a contract splits them into calls, passing the last next_state.state_hash of one as state0 of the next. */
int32_t bzk_contract_updates_check(bzk_ctx* ctx, const bzk_contract_desc* c, const uint8_t* updates, uint64_t len, const uint64_t* count, uint64_t m,
                                   uint64_t height0, const uint8_t state0[32], uint8_t* ok, uint8_t* aux_out, uint8_t* commit_out);
/* Host only, parses and nothing else: for n Transaction / TransactionAndDelta records (form: BZK_L1_FORM_*) lists every ContractUpdate of every
 * UpdateContract whose contract_id equals the given scalar.  spans_out: up to cap entries of three words (transaction index, offset in txs,
 * length); *n_out = the number found, even beyond cap (set to 0 before parsing: that is what a refused call leaves there; spans_out is not
 * written then).  Refusals as bzk_l1_tx_verify_batch.  With it a caller goes from
 * bzk_block_bodies_check's input to bzk_contract_updates_check's. */
int32_t bzk_l1_tx_updates(const uint8_t* txs, uint64_t len, uint64_t n, uint32_t form, const uint8_t contract_id[32], uint64_t* spans_out, uint64_t cap,
                          uint64_t* n_out);
/* Its sibling for the state step: for every UpdateContract of the given contract, four words - transaction index, offset of the ZkDeltaPairs body
 * in txs, its length, and its source: 0 = `delta` inside the transaction, 1 = the record's `state_delta` (form TransactionAndDelta, `delta` None),
 * 2 with length 0 = neither is present (StateNotGiven).  Same parser, same refusals, same cap / n_out rule.  The spans are what
 * bzk_state_update_chain_bincode takes; its claims are each transaction's last next_state. */
int32_t bzk_l1_tx_deltas(const uint8_t* txs, uint64_t len, uint64_t n, uint32_t form, const uint8_t contract_id[32], uint64_t* spans_out, uint64_t cap,
                         uint64_t* n_out);

/* ---- K2: dense 4-ary ZkState tree re-hash ----------------------------------------------------
 * Root of `ZkStateModel::List{log4_size, Scalar}` with every leaf present, as
 * `ZkStateBuilder::compress` / `KvStoreStateManager::root` would give (src/zk/state/mod.rs:66-90,
 * 274-283, 310-420: node = H(c0,c1,c2,c3)).  leaves: 4^log4 scalars.  nodes_opt (may be NULL):
 * receives all internal nodes in the reference's heap order, index (4^k-1)/3 + i for node i of
 * depth k (src/zk/state/mod.rs:355,382-383), root at index 0; (4^log4-1)/3 scalars. */
int32_t bzk_merkle4_root(bzk_ctx* ctx, const uint8_t* leaves, uint32_t log4_size, uint8_t root[32], uint8_t* nodes_opt);
int32_t bzk_merkle4_root_dev(bzk_ctx* ctx, const void* leaves_dev, uint32_t log4_size, uint8_t root[32], void* nodes_opt_dev);

/* Device-resident tree with batched updates and proofs: the level loop of
 * `KvStoreStateManager::set_data` (src/zk/state/mod.rs:310-420) and `prove` (218-264) for a dense
 * `List{log4_size, Scalar}` kept in HBM: (4^(log4+1)-1)/3 scalars, all levels in heap order (node i of depth k at
 * (4^k-1)/3 + i, leaves at depth log4).  log4 <= 15 (4^15 leaves = 46 GB: an account tree of the production size fits).
 *   create : from 4^log4 leaves in device memory, or (leaves_dev NULL) the empty tree of `default_leaf`
 *   update : n (index, leaf) pairs from host memory; re-hashes each affected parent once per level; a later entry
 *            for the same index wins
 *   prove  : for each of n indices log4 sibling triples, leaf level first, index order, self left out
 *            (= the `Vec<[ZkScalar; 3]>` the circuits take); out = n * log4 * 96 bytes */
typedef struct bzk_tree4 bzk_tree4;
int32_t bzk_tree4_create(bzk_ctx* ctx, uint32_t log4_size, const void* leaves_dev, const uint8_t default_leaf[32], bzk_tree4** out);
void    bzk_tree4_free(bzk_ctx* ctx, bzk_tree4* tree);
int32_t bzk_tree4_root(bzk_ctx* ctx, const bzk_tree4* tree, uint8_t root[32]);
int32_t bzk_tree4_update(bzk_ctx* ctx, bzk_tree4* tree, const uint64_t* indices, const uint8_t* leaves, uint64_t n);
int32_t bzk_tree4_prove(bzk_ctx* ctx, const bzk_tree4* tree, const uint64_t* indices, uint64_t n, uint8_t* out);
int32_t bzk_tree4_node(bzk_ctx* ctx, const bzk_tree4* tree, uint32_t depth, uint64_t index, uint8_t out[32]);

/* Device-resident MPN ACCOUNT STATE (second half): the production state model
 *   List{log4_tree, Struct{tx_nonce, withdraw_nonce, pub_x, pub_y, List{log4_token_tree, Struct{token_id, balance}}}}
 * (`MpnConfig::state_model`, src/mpn/mod.rs:218-241) with the batched forms of `KvStoreStateManager::set_mpn_account`
 * (src/zk/state/mod.rs:158-208), `get_mpn_account` (93-137) and `prove` (218-264).  The account level is a dense tree of leaf
 * hashes H5(nonce, wnonce, x, y, tokens_root) in HBM (46 GB at log4_tree = 15); account contents and token sub-trees exist for
 * populated accounts only (`capacity` of them; BZK_E_ALLOC beyond).  All scalars: 32-byte Montgomery.
 *   set_accounts : n DISTINCT accounts; cells = n x 4 scalars (nonce, withdraw nonce, x, y); account a's token updates are
 *                  entries tok_off[a] .. tok_off[a+1] of tok_index (slot < 4^log4_token_tree, distinct per account) and
 *                  tok_vals (token_id, balance); slots not named keep their contents, as in the reference
 *   get_accounts : per account 5 + 2 * 4^T scalars: the 4 cells, tokens_root (`MpnAccount::tokens_hash`), then every token slot
 *   prove        : log4_tree sibling triples per account (the transitions' `proof` / `src_proof` / `dst_proof`)
 *   prove_token  : log4_token_tree sibling triples per (account, token slot) (the `*_balance_proof`s) */
/* `ZkStateModel::compress` of a DENSE MPN-shaped state resident in HBM (BASELINE configs[4], secondary instance): cells_dev = 4^L x 4
 * scalars, tokens_dev = 4^L x 4^T x 2 scalars; one dense launch per level (H2 token slots, T x H4, H5 per account, L x H4). L <= 12. */
int32_t bzk_mpn_state_compress_dev(bzk_ctx* ctx, uint32_t log4_tree, uint32_t log4_token_tree, const void* cells_dev, const void* tokens_dev,
                                   uint8_t root[32]);
typedef struct bzk_mpn_tree bzk_mpn_tree;
int32_t bzk_mpn_tree_create(bzk_ctx* ctx, uint32_t log4_tree, uint32_t log4_token_tree, uint64_t capacity, bzk_mpn_tree** out);
void    bzk_mpn_tree_free(bzk_ctx* ctx, bzk_mpn_tree* tree);
int32_t bzk_mpn_tree_root(bzk_ctx* ctx, const bzk_mpn_tree* tree, uint8_t root[32]);
uint64_t bzk_mpn_tree_accounts(const bzk_mpn_tree* tree);
int32_t bzk_mpn_tree_set_accounts(bzk_ctx* ctx, bzk_mpn_tree* tree, const uint64_t* indices, const uint8_t* cells, const uint64_t* tok_off,
                                  const uint64_t* tok_index, const uint8_t* tok_vals, uint64_t n);
int32_t bzk_mpn_tree_get_accounts(bzk_ctx* ctx, const bzk_mpn_tree* tree, const uint64_t* indices, uint64_t n, uint8_t* out);
int32_t bzk_mpn_tree_prove(bzk_ctx* ctx, const bzk_mpn_tree* tree, const uint64_t* indices, uint64_t n, uint8_t* out);
int32_t bzk_mpn_tree_prove_token(bzk_ctx* ctx, const bzk_mpn_tree* tree, const uint64_t* account_indices, const uint64_t* token_indices,
                                 uint64_t n, uint8_t* out);

/* General seam `ZkStateModel::compress::<H>(&data)` (src/zk/mod.rs:392-399; `ZkStateBuilder::{batch_set, compress}`
 * src/zk/state/mod.rs:66-90 over `set_data` 310-420): ANY nesting of Scalar / Struct{field_types} / List{log4_size, item_type}
 * (src/zk/mod.rs:332-345) over SPARSE (ZkDataLocator, ZkScalar) pairs, untouched sub-trees at `compress_default` (401-423).  The
 * touched part of the state is laid out on the host, grouped by (height, arity), and every group is one batched Poseidon launch.
 *   model          bincode(ZkStateModel) (u32 tags 0 Scalar / 1 Struct + Vec / 2 List + u8 + Box)
 *   loc_off, loc   CSR of the n locators: pair i's indices are loc[loc_off[i] .. loc_off[i + 1])
 *   values         n x 32-byte Montgomery scalars
 *   state_hash, state_size = the two fields of `ZkCompressedState` (size = non-zero scalars, as set_data counts them)
 * BZK_E_ARG where the reference returns LocatorError / NonScalarLocatorError (or panics): a locator that does not end at a
 * scalar, an index >= 4^log4_size or >= the number of fields, a repeated locator, a struct with 0 or > 16 fields (`is_valid`).
 * _bincode: pairs = bincode(ZkDataPairs), out = bincode(ZkCompressedState) (40 B) - what a Rust host holds already.
 * bzk_state_model_default = `compress_default` (host). */
int32_t bzk_state_compress(bzk_ctx* ctx, const uint8_t* model, uint64_t model_len, const uint64_t* loc_off, const uint64_t* loc,
                           const uint8_t* values, uint64_t n, uint8_t state_hash[32], uint64_t* state_size);
int32_t bzk_state_compress_bincode(bzk_ctx* ctx, const uint8_t* model, uint64_t model_len, const uint8_t* pairs, uint64_t pairs_len,
                                   uint8_t compressed_out[40]);
int32_t bzk_state_model_default(const uint8_t* model, uint64_t model_len, uint8_t out[32]);

/* PERSISTENT device state of one contract, any model: `KvStoreStateManager::{update_contract, set_data, get_data, prove, root}`
 * (src/zk/state/mod.rs:286-308, 310-420, 422-438, 218-264, 274-284) with the values resident in HBM.  The reference walks
 * root-wards once per written scalar, one hash and four KV reads per level; here one update is ONE plan - the union of the
 * root-ward paths of every written scalar, each node once, grouped by (height, arity): per group one gather, one batched
 * Poseidon launch, one scatter, in place on the device.  Only the written scalars go up, only the root comes back.
 *   bzk_state_update   = `update_contract(db, id, &ZkDeltaPairs, target_height)`: n (locator, value) pairs, a zero value = the
 *                        reference's `None` (remove).  All or nothing: every locator is checked before a slot changes.
 *                        state_hash / state_size = the new `ZkCompressedState` (either may be NULL).
 *                        prev_values_out (n x 32 B, or NULL) = what the named scalars held before, zero where nothing was stored:
 *                        the rollback delta `ZkState::push_delta` records (src/zk/mod.rs:521-530); feeding it back undoes the update.
 *   _bincode           delta = bincode(ZkDeltaPairs) (HashMap<ZkDataLocator, Option<ZkScalar>>), out = bincode(ZkCompressedState)
 *   bzk_state_root     = `root` (+ `height_of`)
 *   bzk_state_get      = `get_data` for n locators: scalar, or the value of the struct / list named; defaults where untouched
 *   bzk_state_prove    = `prove(db, id, tree_loc, index)` for n indices of ONE list: per index log4_size x 3 scalars, leaf level
 *                        first, the three siblings of a level in ascending position (`Vec<[ZkScalar; 3]>`)
 * Errors as bzk_state_compress (BZK_E_ARG + bzk_last_error(ctx) naming the reference's error); BZK_E_DEVICE after a device
 * failure in the middle of an update (the handle is then unusable).  A handle is bound to its ctx; one thread at a time. */
typedef struct bzk_state bzk_state;
int32_t bzk_state_create(bzk_ctx* ctx, const uint8_t* model, uint64_t model_len, bzk_state** out);
void bzk_state_free(bzk_state* st);
int32_t bzk_state_update(bzk_state* st, const uint64_t* loc_off, const uint64_t* loc, const uint8_t* values, uint64_t n,
                         uint64_t target_height, uint8_t state_hash[32], uint64_t* state_size, uint8_t* prev_values_out);
int32_t bzk_state_update_bincode(bzk_state* st, const uint8_t* delta, uint64_t delta_len, uint64_t target_height,
                                 uint8_t compressed_out[40]);
int32_t bzk_state_root(bzk_state* st, uint8_t state_hash[32], uint64_t* state_size, uint64_t* height);
int32_t bzk_state_get(bzk_state* st, const uint64_t* loc_off, const uint64_t* loc, uint64_t n, uint8_t* values_out);
int32_t bzk_state_prove(bzk_state* st, const uint64_t* tree_loc, uint64_t tree_loc_len, const uint64_t* indices, uint64_t n,
                        uint8_t* proof_out, uint32_t* log4_size);
int32_t bzk_state_stats(bzk_state* st, uint64_t* slots, uint64_t* device_bytes, uint64_t* keys);

/* A CHAIN of m deltas in one pass (`update_contract/mod.rs:129-144` per block: apply the transaction's ZkDeltaPairs, then require
 * root == cont_account.compressed_state).  Exactly this loop: for j = 0 .. m - 1 call bzk_state_update(delta j, target_heights[j]), compare the
 * 40 bytes of bincode(ZkCompressedState) (hash, then size) with claims[j], stop at the first delta that is refused or does not match; a delta that
 * stops the loop leaves no trace.  All deltas go through the tree together - one launch per (level, arity) over every (node, time) pair of a
 * round - and nothing in the value store changes before the roots have been compared.
 *   delta_off        m + 1 offsets in PAIRS: delta j is pairs delta_off[j] .. delta_off[j + 1] of loc_off / loc / values (as bzk_state_update)
 *   claims           m x 40 bytes, or NULL: nothing can mismatch
 *   round_versions   0 = 2^22: whole deltas share a round while their written scalars + hashed nodes stay at most this; a larger delta runs alone
 *   states_out       m x 40: for an applied and for a mismatching delta the state it produces; zeros from a refused delta onwards
 *   verdict          m x BZK_CHAIN_*;  *applied = the deltas that are part of the state now.  Afterwards the handle is indistinguishable from
 *                    one that received the first *applied deltas through bzk_state_update (root, size, height, get, prove, keys)
 *   prev_values_out  pairs x 32 or NULL: for every pair of an applied delta what that scalar held just before its delta (the per-block rollback
 *                    of `ZkState::push_delta`); zeros elsewhere
 * An empty delta moves the height only and repeats the state before it.  BZK_OK whenever the verdicts tell the story: a refused delta is a
 * verdict, bzk_last_refusal / bzk_last_error name its reason and its index.  BZK_E_ARG for call-level faults only, nothing changed: NULL pointers
 * with m > 0, offsets that do not ascend.  m = 0 is a no-op.  BZK_E_DEVICE poisons the handle.
 * _bincode: m bincode(ZkDeltaPairs) blobs back to back, blob j at delta_byte_off[j] .. delta_byte_off[j + 1], read by bzk_state_update_bincode's
 * decoder; a blob that does not decode is REFUSED.
 * Measured (DESIGN 3.15, 1 024 pairs per delta at the production depth): ONE delta through this call costs what a bzk_state_update of it costs
 * (0.8 - 1.3 x across runs) - the same 20 dependent launches, and the versioning costs the host what the fused kernel saves; 16 deltas cost 2.6 x
 * less than 16 calls, 64 and more 3.1 - 3.2 x less, bounded by the host's planning.  With one or two deltas keep bzk_state_update. */
#define BZK_CHAIN_APPLIED     0u  /* the delta is part of the state now */
#define BZK_CHAIN_MISMATCH    1u  /* applied alone it gives another ZkCompressedState than claimed (BlockchainError::InvalidState) */
#define BZK_CHAIN_REFUSED     2u  /* bzk_state_update would refuse it (locator errors, duplicate, non-canonical value) */
#define BZK_CHAIN_NOT_REACHED 3u  /* behind the first delta that was not applied */
int32_t bzk_state_update_chain(bzk_state* st, uint64_t m, const uint64_t* delta_off, const uint64_t* loc_off, const uint64_t* loc,
                               const uint8_t* values, const uint64_t* target_heights, const uint8_t* claims, uint64_t round_versions,
                               uint8_t* states_out, uint8_t* verdict, uint64_t* applied, uint8_t* prev_values_out);
int32_t bzk_state_update_chain_bincode(bzk_state* st, uint64_t m, const uint8_t* deltas, const uint64_t* delta_byte_off,
                                       const uint64_t* target_heights, const uint8_t* claims, uint64_t round_versions, uint8_t* states_out,
                                       uint8_t* verdict, uint64_t* applied);

/* ---- K3: radix-2 NTT over Fr -----------------------------------------------------------------
 * bellman 0.14 `EvaluationDomain::{fft, ifft, coset_fft, icoset_fft}` (third-party crate; reached
 * from `create_random_proof`, src/mpn/circuits/test.rs:135,175,215).  In place, natural order in and
 * out.  omega = 7^((r-1)/2^32)^(2^(32-log_n)); coset shift g = 7.
 *   inverse=0,coset=0: a_k = sum_j a_j w^jk          inverse=1,coset=0: ... w^-jk / n
 *   inverse=0,coset=1: scale a_j by g^j, then fft     inverse=1,coset=1: ifft, then scale by g^-j */
int32_t bzk_ntt(bzk_ctx* ctx, uint8_t* data, uint32_t log_n, int32_t inverse, int32_t coset);
int32_t bzk_ntt_dev(bzk_ctx* ctx, void* data_dev, uint32_t log_n, int32_t inverse, int32_t coset);

/* ---- K4 / K5: Pippenger multi-scalar multiplication ------------------------------------------
 * bellman 0.14 `multiexp` over G1 / G2 (third-party; the `h`, `l`, `a`, `b_g1`, `b_g2` queries of
 * `create_proof`).  result = sum_i scalar_i * base_i, written packed (97 / 193 B).
 * bases: raw affine, never the identity (bellman drops identity points from the CRS). */
int32_t bzk_msm_g1(bzk_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, uint64_t n, uint32_t flags, uint8_t out[97]);
int32_t bzk_msm_g1_dev(bzk_ctx* ctx, const void* bases_dev, const void* scalars_dev, uint64_t n, uint32_t flags, uint8_t out[97]);
int32_t bzk_msm_g2(bzk_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, uint64_t n, uint32_t flags, uint8_t out[193]);
int32_t bzk_msm_g2_dev(bzk_ctx* ctx, const void* bases_dev, const void* scalars_dev, uint64_t n, uint32_t flags, uint8_t out[193]);

/* Sharded form for multi-GPU: this rank computes only windows
 * [w_begin, w_end) of the W = bzk_msm_window_count(n) signed c-bit windows and returns their partial
 * sum  sum_w 2^(c*w) * S_w  as a packed point; the partial sums of all ranks add up to the MSM.
 * Ranks exchange the 97/193-byte partials as raw bytes (RCCL all-gather) and fold them with
 * bzk_g1_sum / bzk_g2_sum - RCCL itself cannot add curve points. */
uint32_t bzk_msm_window_count(uint64_t n);
int32_t bzk_msm_g1_windows_dev(bzk_ctx* ctx, const void* bases_dev, const void* scalars_dev, uint64_t n, uint32_t flags,
                               uint32_t w_begin, uint32_t w_end, uint8_t out[97]);
int32_t bzk_msm_g2_windows_dev(bzk_ctx* ctx, const void* bases_dev, const void* scalars_dev, uint64_t n, uint32_t flags,
                               uint32_t w_begin, uint32_t w_end, uint8_t out[193]);
int32_t bzk_g1_sum(const uint8_t* packed_points, uint32_t count, uint8_t out[97]);   /* host, tiny */
int32_t bzk_g2_sum(const uint8_t* packed_points, uint32_t count, uint8_t out[193]);

/* ---- Groth16 prove (a4-a7) --------------------------------------------------------------------
 * bellman 0.14 `groth16::create_proof(circuit, params, r, s)` after synthesis (third-party; call
 * sites src/mpn/circuits/test.rs:135,175,215): 3 iNTT + 3 coset NTT + pointwise (a*b-c)/Z + 1 inverse
 * coset NTT -> h; MSMs over the h / l / a / b_g1 / b_g2 queries; assembly of (A, B, C).
 * Output = the 387 bytes of `Groth16Proof` (src/zk/groth16/mod.rs:33-38), i.e. the payload of
 * `ZkProof::Groth16` (src/zk/mod.rs:646-651) that `groth16_verify` (src/zk/groth16/mod.rs:67-121)
 * accepts.
 *
 * CRS layout (= bellman `Parameters`, identity points dropped): variables are numbered inputs first
 * (index 0 = ONE) then aux.  a / b_g1 / b_g2 hold ONLY the variables whose density flag is set, in
 * variable order (a_density[v] = v occurs in some A row; b_density likewise). */
typedef struct bzk_params bzk_params;
typedef struct {
    uint32_t n_in, n_aux, log_m; /* m = 2^log_m >= number of constraints */
    uint32_t n_a, n_b;           /* popcount of a_density / b_density */
    const uint8_t* vk;           /* 870 B: alpha_g1|beta_g1|beta_g2|gamma_g2|delta_g1|delta_g2, packed */
    const uint8_t* h;            /* (m-1) raw G1 */
    const uint8_t* l;            /* n_aux raw G1 */
    const uint8_t* a;            /* n_a raw G1 */
    const uint8_t* b_g1;         /* n_b raw G1 */
    const uint8_t* b_g2;         /* n_b raw G2 */
    const uint8_t* a_density;    /* n_in + n_aux bytes, 0/1 */
    const uint8_t* b_density;    /* n_in + n_aux bytes, 0/1 */
} bzk_params_desc;
typedef struct {
    const uint8_t* z;            /* (n_in + n_aux) scalars: inputs (z[0] = 1) then aux, Montgomery */
    const uint8_t* az;           /* n_rows scalars: <A_k, z> per constraint */
    const uint8_t* bz;
    const uint8_t* cz;
    uint64_t n_rows;             /* number of constraints incl. bellman's n_in trailing `input*0=0` rows */
    uint64_t n_vars;             /* scalars behind `z`: must equal the params' n_in + n_aux, else BZK_E_ARG (an assignment
                                    of another circuit shape is refused, never read out of bounds) */
} bzk_assignment;
/* uploads the CRS to HBM once (host pointers in the descriptor are not retained) */
int32_t bzk_params_load(bzk_ctx* ctx, const bzk_params_desc* desc, bzk_params** out);
void bzk_params_free(bzk_ctx* ctx, bzk_params* params);
/* A further prover SLOT over the same device-resident CRS: `bzk_groth16_prove` is not re-entrant per params handle, which owns its
 * per-proof device scratch,, so a prover that keeps several proofs in flight on one GPU (their latency-bound phases hide under
 * each other's accumulation) uses one ctx + one slot per thread.  Slots SHARE the uploaded CRS, its resident internal forms and the
 * h table (reference-counted; the last bzk_params_free releases them): n slots cost n x scratch, not n x CRS. */
int32_t bzk_params_slot(bzk_ctx* ctx, const bzk_params* params, bzk_params** out);
/* The first proof over a CRS builds, ONCE per device and only where hipMemGetInfo shows room for them beside a workspace reserve,
 * the resident internal forms of l / a / b_g1 / b_g2 (no base conversion inside a proof) and, for 2^16 .. 2^24 domains, a static
 * table of the h query (13 levels: 1.5 GB at 2^20, 24 GB at the production 2^24 - one per DEVICE, shared by the slots).  bzk_params_h_table(.., 1) builds that table now, for any domain size that
 * fits; (.., 0) drops it / keeps the first proof from building it (only while this handle is the CRS's sole slot).  Environment:
 * BZK_PROVE_H_TABLE=0, BZK_PROVE_H_TABLE_MAX_LOG, BZK_PROVE_RESIDENT_BASES=0. */
int32_t bzk_params_h_table(bzk_ctx* ctx, bzk_params* params, int32_t on);
/* The resident query sets of a parameter set's CRS, once its first proof (or bzk_params_h_table) has prepared them: *sets = how many are held,
 * *device_bytes = their HBM, *table_bytes = HBM of window tables among them (bzk_msm_bases_table_info) - 0: the prover's MSMs are
 * throughput-flagged or de-duplicated and never run from such a table, so its sets are loaded without one whatever BZK_MSM_BASES_TABLE says. */
int32_t bzk_params_resident_info(bzk_params* params, uint32_t* sets, uint64_t* device_bytes, uint64_t* table_bytes);
/* r, s: Montgomery scalars (the prover's blinding factors; bellman draws them from the rng) */
int32_t bzk_groth16_prove(bzk_ctx* ctx, bzk_params* params, const bzk_assignment* asg, const uint8_t r[32],
                          const uint8_t s[32], uint8_t proof_out[387]);
/* bellman's `groth16::Parameters<Bls12>` file format (third-party crate; the proving keys a real network ships and its
 * external prover loads, README.md:26-28; dev networks generate theirs in memory, src/config/blockchain.rs:355-417):
 *   Parameters::write = VerifyingKey::write | u32-BE n, h.. | u32-BE n, l.. | u32-BE n, a.. | u32-BE n, b_g1.. | u32-BE n, b_g2..
 * with `to_uncompressed` points (48-byte big-endian canonical coordinates, G2 as c1 | c0, flag bits in byte 0).  Host code.
 *   info   : lengths of ic, h, l, a, b_g1, b_g2 and the bytes consumed
 *   decode : -> vk870 (packed alpha_g1 | beta_g1 | beta_g2 | gamma_g2 | delta_g1 | delta_g2), ic (packed 97 B each), raw
 *            Montgomery h / l / a / b_g1 (96 B) and b_g2 (192 B); canonical-range and on-curve checks, infinity refused in
 *            the queries as `Parameters::read` does; threads 0 = all cores
 *   encode : the inverse; out NULL = size query
 *   bzk_params_load_bellman : parse + upload for a prover.  The file does not say which variables the a / b queries belong
 *            to (bellman derives that from the circuit): pass the density maps of the circuit shape (bzk_r1cs_data views 4, 5
 *            of the empty circuit); every length is checked against them.  vk_out (optional): bincode(Groth16VerifyingKey). */
int32_t bzk_bellman_params_info(const uint8_t* bytes, uint64_t len, uint64_t info[7]);
int32_t bzk_bellman_params_decode(const uint8_t* bytes, uint64_t len, uint8_t* vk870, uint8_t* ic, uint8_t* h, uint8_t* l, uint8_t* a,
                                  uint8_t* b_g1, uint8_t* b_g2, int32_t threads);
int32_t bzk_bellman_params_encode(const uint8_t vk870[870], const uint8_t* ic, uint64_t n_ic, const uint8_t* h, uint64_t n_h, const uint8_t* l,
                                  uint64_t n_l, const uint8_t* a, uint64_t n_a, const uint8_t* b_g1, const uint8_t* b_g2, uint64_t n_b,
                                  uint8_t* out, uint64_t cap, uint64_t* size_out);
int32_t bzk_params_load_bellman(bzk_ctx* ctx, const uint8_t* bytes, uint64_t len, uint32_t n_in, uint32_t n_aux, const uint8_t* a_density,
                                const uint8_t* b_density, bzk_params** out, uint8_t* vk_out, uint64_t vk_cap);
/* `groth16_verify` (src/zk/groth16/mod.rs:67-121; bellman `verify_proof`): host code, no GPU.  vk = bincode(Groth16VerifyingKey)
 * (870 + 8 + 97 n bytes, n = n_inputs + 1); inputs = n_inputs Montgomery scalars (the reference passes commitment, height, state,
 * aux_data, next_state).  Returns 1 (verifies), 0 (does not - incl. malformed or off-curve points, for which the reference returns
 * false), negative on bad arguments.  ~20 ms on one core. */
int32_t bzk_groth16_verify(const uint8_t* vk, uint64_t vk_len, const uint8_t* inputs, uint32_t n_inputs, const uint8_t proof[387]);
/* The same check for n proofs of ONE verifying key (the caller groups its proofs by circuit; MPN has three keys per contract), one GPU lane per
 * proof: what `apply_tx/update_contract/mod.rs:100` runs per ContractUpdate and `MpnWork::verify` (src/mpn/mod.rs:281-295) per posted solution.
 * inputs = n x n_inputs Montgomery scalars, proofs = n x 387 bytes; ok[i] = bzk_groth16_verify(vk, vk_len, inputs + 32 n_inputs i, n_inputs,
 * proofs + 387 i) for any bytes whatever: 1 verifies; 0 does not, a coordinate's limbs are >= p, a point is off its curve, an input's limbs are
 * >= r, or a line's slope had a zero denominator.  A key the single call refuses with 0 (n_ic != n_inputs + 1, a wrong vk_len, a key point off
 * its curve or out of range) gives ok[i] = 0 for all i and BZK_OK.  Null pointers with n > 0 or vk_len < 878: BZK_E_ARG, nothing written;
 * n = 0: BZK_OK.  Once per call the host unpacks the key and builds its window tables, the line coefficients of -gamma and -delta and the
 * constant Miller value of (-alpha, beta); three kernels (prepare, Miller loop, final exponentiation) then run rounds of at most 2^16 proofs.
 * ctx = NULL runs the same per-proof functions over the host field on the host's threads; with a context, n_inputs > 16 is routed to that same
 * host-thread path (same verdicts, no refusal).  The _dev form takes device pointers (vk stays a host pointer) and needs a context. */
int32_t bzk_groth16_verify_batch(bzk_ctx* ctx, const uint8_t* vk, uint64_t vk_len, const uint8_t* inputs, uint32_t n_inputs,
                                 const uint8_t* proofs, uint64_t n, uint8_t* ok);
int32_t bzk_groth16_verify_batch_dev(bzk_ctx* ctx, const uint8_t* vk, uint64_t vk_len, const void* inputs_dev, uint32_t n_inputs,
                                     const void* proofs_dev, uint64_t n, void* ok_dev);
/* The same check for proofs of SEVERAL keys in one call (a block's Deposit, Withdraw and Update proofs have three): every verdict is what
 * bzk_groth16_verify_batch says about that proof under its key, but the device runs ONE set of launches per round of 2^16 lanes instead of one
 * per key - the lanes of all keys side by side, every key's proofs padded to whole blocks of 64 - so a call of a few thousand proofs costs one
 * lane's chain of dependent products, not one per key.  Key k is the bytes vks[vk_off[k] .. vk_off[k + 1]) (vk_off: n_keys + 1 ascending
 * offsets) with n_inputs[k] inputs.
 * bzk_groth16_verify_batch_keys: n proofs in any order, proof i of key key_of[i]; inputs are packed in proof order (proof i holds
 * 32 n_inputs[key_of[i]] bytes), proofs = n x 387 bytes; the host groups the rows by key (a stable counting sort), stages them round by round
 * and returns ok[i] in the caller's order.  ctx = NULL runs the per-proof functions on the host's threads, all proofs in one task loop.
 * bzk_groth16_verify_groups_dev: the rows already grouped in device memory - group g is counts[g] proofs of key g, the groups' inputs, proofs
 * and verdict bytes each contiguous, group after group (two groups may name the same key bytes; a count of 0 is legal anywhere); needs a context.
 * A key the single call refuses gives 0 for ITS proofs only; a key of more than 16 inputs takes the host-thread route (on copies in the device
 * form) while the other keys' proofs run on the device.  BZK_E_ARG, nothing written: key_of[i] >= n_keys, vk_off not ascending, a key shorter
 * than 878 bytes, n_keys = 0 with n > 0, a null pointer with n > 0.  n = 0 (all counts 0): BZK_OK, nothing touched. */
int32_t bzk_groth16_verify_batch_keys(bzk_ctx* ctx, uint32_t n_keys, const uint8_t* vks, const uint64_t* vk_off, const uint32_t* n_inputs,
                                      const uint32_t* key_of, const uint8_t* inputs, const uint8_t* proofs, uint64_t n, uint8_t* ok);
int32_t bzk_groth16_verify_groups_dev(bzk_ctx* ctx, uint32_t n_groups, const uint8_t* vks, const uint64_t* vk_off, const uint32_t* n_inputs,
                                      const uint64_t* counts, const void* inputs_dev, const void* proofs_dev, void* ok_dev);
/* Subgroup membership of n raw points (little-endian Montgomery limbs: G1 x | y = 96 B, G2 x.c0 | x.c1 | y.c0 | y.c1 = 192 B; what
 * bzk_bellman_params_decode emits), one GPU lane per point: the third check of bls12_381 `from_uncompressed` after canonical range and the
 * curve equation.  ok[i] = 1: in the order-r subgroup; 0: on the curve but outside it; 2: not a valid finite curve point (a coordinate's limbs
 * >= p, or off the curve).  inf (n bytes, may be NULL): a record with inf[i] != 0 is the identity, its bytes are not read and ok[i] = 1.
 * G1: [X]([X] P) == (BETA x, -y); G2: [X] P == psi(P); X = 0xd201000000010000, the ladders by complete projective formulas, so every
 * point - of any order - runs the same steps.  Null pts / ok with n > 0: BZK_E_ARG, nothing written; n = 0: BZK_OK.  ctx = NULL runs the same
 * per-point functions over the host field on the host's threads.  With a context the records are staged in rounds of 2^18 points (the workspace
 * holds one round: records, flags and verdict bytes).  The _dev
 * forms take device pointers (pts 4-byte aligned), need a context, and launch rounds of 2^18 points.  Synchronises. */
int32_t bzk_g1_subgroup_check_batch(bzk_ctx* ctx, const uint8_t* pts, const uint8_t* inf, uint64_t n, uint8_t* ok);
int32_t bzk_g1_subgroup_check_batch_dev(bzk_ctx* ctx, const void* pts_dev, const void* inf_dev, uint64_t n, void* ok_dev);
int32_t bzk_g2_subgroup_check_batch(bzk_ctx* ctx, const uint8_t* pts, const uint8_t* inf, uint64_t n, uint8_t* ok);
int32_t bzk_g2_subgroup_check_batch_dev(bzk_ctx* ctx, const void* pts_dev, const void* inf_dev, uint64_t n, void* ok_dev);
/* bellman `Parameters::read(reader, checked = true)` as a verdict: everything bzk_bellman_params_decode checks, plus the subgroup check of the
 * six verifying-key points, of ic and of the five queries.  Returns 1 (every point passes), 0 (one does not; report says which), negative on
 * bad arguments (bytes or report NULL) or a device failure.  report = {array: 0 vk head (alpha_g1, beta_g1, beta_g2, gamma_g2, delta_g1,
 * delta_g2), 1 ic, 2 h, 3 l, 4 a, 5 b_g1, 6 b_g2, 7 the array lengths do not fit the blob (or, in the loader, the circuit shape); element index;
 * verdict code as above (2 also for the identity inside a query); 0} of the first failure in file order; zeros on success.  The identity passes
 * inside the verifying key and ic, as it does in the decoder.  ctx = NULL: host threads; with a context the queries run on the device.
 * bzk_params_load_bellman_checked: bzk_params_load_bellman with that check - same handle, same vk_out bytes on success; on a failed point
 * BZK_E_ARG, report filled, bzk_last_error naming the array and index, *out NULL.  The queries are checked where bzk_params_load put them (one
 * upload: the kernels read the loaded arrays, and a failure frees the handle again); the verifying key and ic are checked on the host first. */
int32_t bzk_bellman_params_check(bzk_ctx* ctx, const uint8_t* bytes, uint64_t len, uint64_t report[4]);
int32_t bzk_params_load_bellman_checked(bzk_ctx* ctx, const uint8_t* bytes, uint64_t len, uint32_t n_in, uint32_t n_aux, const uint8_t* a_density,
                                        const uint8_t* b_density, bzk_params** out, uint8_t* vk_out, uint64_t vk_cap, uint64_t report[4]);
/* reads a CRS component back (tests): which = 0 vk (870 B), 1 h, 2 l, 3 a, 4 b_g1, 5 b_g2 */
int32_t bzk_params_read(bzk_ctx* ctx, const bzk_params* params, int32_t which, uint8_t* out, uint64_t cap, uint64_t* size_out);

/* CRS generation on the GPU = bellman `generate_parameters(circuit, g1, g2, alpha, beta, gamma, delta, tau)` with
 * g1, g2 the standard generators (the reference's dev-mode CRS: src/config/blockchain.rs:355-417).  The R1CS comes
 * as CSR matrices over flat variable indices (inputs then aux), rows already including bellman's trailing
 * `input_i * 0 = 0` constraints (bzk_r1cs_data views 6-14 of a circuit synthesized with record_matrices).
 * toxic = tau | alpha | beta | gamma | delta (5 x 32 B Montgomery).  vk_out (optional) receives the bincode form of
 * `Groth16VerifyingKey` (src/zk/groth16/mod.rs:22-31): 870 + 8 + 97 * n_in bytes. */
typedef struct {
    uint64_t n_rows;
    const uint32_t* row_ptr; /* n_rows + 1 */
    const uint32_t* col;     /* nnz */
    const uint8_t* val;      /* nnz * 32, Montgomery */
} bzk_csr;
int32_t bzk_groth16_setup(bzk_ctx* ctx, const bzk_csr* A, const bzk_csr* B, const bzk_csr* C, uint32_t n_in, uint32_t n_aux,
                          const uint8_t toxic[160], bzk_params** out_params, uint8_t* vk_out, uint64_t vk_cap);

/* n G1 points times ONE scalar, one GPU lane per point: out[i] = k * pts[i].  pts and out are raw 96-byte records (little-endian Montgomery
 * x | y: what bzk_bellman_params_decode emits and bzk_g1_subgroup_check_batch takes), out in canonical affine; k is one Montgomery Fr scalar
 * (as r and s of bzk_groth16_prove).  An identity result is 96 zero bytes with inf_out[i] = 1 (inf_out: n bytes, may be NULL; 0 for a finite
 * result); a record of 96 zero bytes is read as the identity.  k = 0 is legal: n identities.  The contract covers points of the order-r
 * subgroup - what a checked CRS holds: the scalar is split through the endomorphism X^2 (x, y) = (BETA x, -y), which is multiplication by
 * X^2 only there.  For any other input (outside the subgroup, off the curve, limbs >= p) the output is unspecified; nothing faults, the
 * formulas are the complete ones of the subgroup check and no step depends on the point.  The scalar is recoded once per call on the host
 * and treated as a secret: its host and device copies are overwritten before the call returns.  BZK_E_ARG, nothing written: limbs of k not
 * below r, null pts or out with n > 0.  n = 0: BZK_OK.  ctx = NULL runs the same per-point function over the host field on the host's
 * threads.  With a context the records are staged in rounds of 2^18 points (the workspace holds one round).  The _dev form takes device
 * pointers (4-byte aligned), may run in place (out_dev == pts_dev) and needs a context.  Synchronises. */
int32_t bzk_g1_scale_batch(bzk_ctx* ctx, const uint8_t* pts, uint64_t n, const uint8_t k[32], uint8_t* out, uint8_t* inf_out);
int32_t bzk_g1_scale_batch_dev(bzk_ctx* ctx, const void* pts_dev, uint64_t n, const uint8_t k[32], void* out_dev, void* inf_out_dev);
/* The phase-2 step of a ceremony on a resident key: a NEW handle whose delta is d times the source's.  h' = d^-1 h and l' = d^-1 l by
 * bzk_g1_scale_batch_dev on the source's arrays, a, b_g1 and b_g2 copied device to device, delta_g1' = d delta_g1 and delta_g2' = d delta_g2 on
 * the host; alpha, beta, gamma (and ic, which no handle holds) do not change.  d: one Montgomery Fr scalar, not zero, limbs below r (else
 * BZK_E_ARG); d and d^-1 are overwritten in host and device memory before the call returns.  vk870_out (optional): the new 870-byte head.
 * The source handle, its slots, resident forms and h table are untouched; the new handle builds its own on its first proof.  A device
 * failure frees the new handle (*out NULL).  The result equals bzk_groth16_setup with delta * d byte for byte.
 * This re-keys delta ALONE and is no ceremony: whoever knows tau of a dev-mode CRS recovers (1 / delta') G1 from h'[0] and forges at will. */
int32_t bzk_params_rekey(bzk_ctx* ctx, const bzk_params* params, const uint8_t d[32], bzk_params** out, uint8_t vk870_out[870]);
/* The same step on a bellman `Parameters` blob: decode, re-key, encode.  out NULL: size query (*size_out = the input's consumed length, which is
 * also the output's).  ctx = NULL: host threads; with a context the h and l queries run on the device - the same bytes either way.
 * BZK_E_ARG: d zero or not below r, cap too small, a blob bzk_bellman_params_decode refuses.
 * bzk_bellman_params_rekey_check: is `after` a re-key of `before` by SOME d?  Returns 1, 0, or a negative status as bzk_bellman_params_check,
 * report = {array, index, code, 0} with the same array codes (0 vk head, 1 ic, 2 h, 3 l, 4 a, 5 b_g1, 6 b_g2, 7 lengths).  1 exactly when:
 * both blobs decode and all array lengths agree (else array 7); alpha_g1, beta_g1, beta_g2, gamma_g2, ic, a, b_g1, b_g2 are byte-equal (else
 * the first differing element, code 0); every point of after's h, l, delta_g1, delta_g2 is in the order-r subgroup (else that point and its
 * verdict code - a cofactor component vanishes under the pairing, so the ratio test alone would accept h'_i + T_i); delta is one multiple in
 * both groups, e(delta_g1, G2) = e(G1, delta_g2), before and after (else array 0, index 4 or 5); and e(S(h'), delta_g2') = e(S(h), delta_g2)
 * with S(q) = sum_i rho_i q_i, likewise for l (else array 2 or 3, index 0, code 0).  rho_i = the low 16 bytes of SHA3-256(seed | array code
 * as one byte | LE64(i)) as an integer.  The four sums are device MSMs with a context, host sums without.  The verdict is only as good as
 * the secrecy of seed from whoever made `after`: with seed known, h' can be chosen to cancel inside S. */
int32_t bzk_bellman_params_rekey(bzk_ctx* ctx, const uint8_t* bytes, uint64_t len, const uint8_t d[32], uint8_t* out, uint64_t cap,
                                 uint64_t* size_out);
int32_t bzk_bellman_params_rekey_check(bzk_ctx* ctx, const uint8_t* before, uint64_t before_len, const uint8_t* after, uint64_t after_len,
                                       const uint8_t seed[32], uint64_t report[4]);

/* n points times n DIFFERENT scalars, one GPU lane per point: out[i] = scalars[i] * pts[i], on G1 (raw 96-byte records x | y) and on G2 (raw
 * 192-byte records x.c0 | x.c1 | y.c0 | y.c1), little-endian Montgomery limbs in, canonical affine out - the records the subgroup checks and
 * the one-scalar call above take.  scalars: n x 32 bytes, Montgomery limbs, or plain integers with BZK_F_CANONICAL in flags (other flag bits
 * are ignored).  An identity result is zero bytes with inf_out[i] = 1 (inf_out: n bytes, may be NULL; 0 for a finite result); a record of zero
 * bytes is read as the identity; a zero scalar gives the identity.  The contract covers points of the order-r subgroup (the scalar is split
 * through X^2 (x, y) = (c x, -y), which is multiplication by X^2 only there); for any other input the output is unspecified and nothing faults:
 * the formulas are the complete ones of the subgroup check, every lane runs the same 128 steps and no step depends on the point's value.
 * BZK_E_ARG, nothing written: a scalar whose limbs are not below r (all n are tested first), null pts, scalars or out with n > 0.  n = 0:
 * BZK_OK.  ctx = NULL runs the same per-point function over the host field on the host's threads.  With a context, host records are staged in
 * rounds of 2^18 points.  The _dev forms take device pointers (4-byte aligned, scalars too), may run in place (out_dev == pts_dev) and need a
 * context.  Synchronises.
 * The powers forms: out[i] = c * s^(start + i) * pts[i], the scalars made on the device from a table of s^(2^j) (start + n must not pass
 * 2^64).  c and s are Montgomery scalars with limbs below r (else BZK_E_ARG) and are treated as secrets: the table, and the recoded scalars of
 * every round, are overwritten in host and device memory before the call returns.
 * A throughput implementation: the multiplier is not hardened against timing (lanes skip the additions of their zero bits). */
int32_t bzk_g1_mul_batch(bzk_ctx* ctx, const uint8_t* pts, const uint8_t* scalars, uint64_t n, uint32_t flags, uint8_t* out, uint8_t* inf_out);
int32_t bzk_g1_mul_batch_dev(bzk_ctx* ctx, const void* pts_dev, const void* scalars_dev, uint64_t n, uint32_t flags, void* out_dev,
                             void* inf_out_dev);
int32_t bzk_g2_mul_batch(bzk_ctx* ctx, const uint8_t* pts, const uint8_t* scalars, uint64_t n, uint32_t flags, uint8_t* out, uint8_t* inf_out);
int32_t bzk_g2_mul_batch_dev(bzk_ctx* ctx, const void* pts_dev, const void* scalars_dev, uint64_t n, uint32_t flags, void* out_dev,
                             void* inf_out_dev);
int32_t bzk_g1_mul_powers(bzk_ctx* ctx, const uint8_t* pts, uint64_t n, const uint8_t c[32], const uint8_t s[32], uint64_t start, uint8_t* out,
                          uint8_t* inf_out);
int32_t bzk_g1_mul_powers_dev(bzk_ctx* ctx, const void* pts_dev, uint64_t n, const uint8_t c[32], const uint8_t s[32], uint64_t start,
                              void* out_dev, void* inf_out_dev);
int32_t bzk_g2_mul_powers(bzk_ctx* ctx, const uint8_t* pts, uint64_t n, const uint8_t c[32], const uint8_t s[32], uint64_t start, uint8_t* out,
                          uint8_t* inf_out);
int32_t bzk_g2_mul_powers_dev(bzk_ctx* ctx, const void* pts_dev, uint64_t n, const uint8_t c[32], const uint8_t s[32], uint64_t start,
                              void* out_dev, void* inf_out_dev);
/* A powers-of-tau accumulator (phase 1 of a ceremony) as one flat blob of this library's raw records (no other tool's file format):
 *   "BZKPTAU1" | u32 log_m | u32 0 | tau_g1[2m - 1] | tau_g2[m] | alpha_g1[m] | beta_g1[m] | beta_g2,   m = 2^log_m, log_m in 1 .. 24
 * with tau_g1[i] = tau^i G1, tau_g2[i] = tau^i G2, alpha_g1[i] = alpha tau^i G1, beta_g1[i] = beta tau^i G1, beta_g2 = beta G2.
 * bzk_ptau_size: the blob's length (0 for a log_m outside 1 .. 24).  bzk_ptau_init: the trivial accumulator, every entry its group's generator
 * (BZK_E_ARG: out NULL, bad log_m, cap too small).
 * bzk_ptau_contribute: out = in with tau, alpha, beta multiplied by the three secrets (tau | alpha | beta, Montgomery, limbs below r, none
 * zero - else BZK_E_ARG, as for a blob that does not parse or a cap below its size; nothing written): five calls of the powers form above, on
 * the device with a context, on host threads without; beta_g2 and key_out = tau G2 | alpha G2 | beta G2 (raw records, the public key of this
 * contribution) on the host.  out may be in.  The secrets are the caller's to overwrite; every copy this call makes is overwritten.
 * bzk_ptau_check: returns 1, 0 or a negative status; report = {array, index, code, 0} names the first failure (zeros on success), array =
 * 0 header or lengths (index 1: of before), 1 tau_g1, 2 tau_g2, 3 alpha_g1, 4 beta_g1, 5 beta_g2, 6 key.  1 exactly when, in this order: after
 * parses (and before, with the same log_m); every point of after passes the subgroup check above, the identity refused (else that point and its
 * verdict code); tau_g1[0] and tau_g2[0] are the generators byte for byte; with rho_i as in the re-key check (array code as the code byte)
 * e(S1, G2) = e(S0, tau_g2[1]) for S0 = sum_i rho_i q[i], S1 = sum_i rho_i q[i + 1] over q = tau_g1, then e(tau_g1[1], T0) = e(G1, T1) for the
 * same sums over tau_g2, then the first form over alpha_g1 and over beta_g1 (else that array, index 0); e(beta_g1[0], G2) = e(G1, beta_g2)
 * (else array 5); and, with before (key NULL exactly when before is, else BZK_E_ARG), for k = tau, alpha, beta: the key point is in the G2
 * subgroup and e(after.x, G2) = e(before.x, key_k) for x = tau_g1[1], alpha_g1[0], beta_g1[0] (else array 6, index k).  The sums are device
 * MSMs with a context, host sums without.
 * The verdict is only as good as the secrecy of seed from whoever made `after`.  There is no proof of knowledge of the key's exponents, no
 * transcript hash and no hardening of the multiplier against timing: a throughput implementation of the arithmetic, not a ceremony client. */
uint64_t bzk_ptau_size(uint32_t log_m);
int32_t bzk_ptau_init(uint32_t log_m, uint8_t* out, uint64_t cap);
int32_t bzk_ptau_contribute(bzk_ctx* ctx, const uint8_t* in, uint64_t len, const uint8_t secrets[96], uint8_t* out, uint64_t cap,
                            uint8_t key_out[576]);
int32_t bzk_ptau_check(bzk_ctx* ctx, const uint8_t* before, uint64_t before_len, const uint8_t key[576], const uint8_t* after, uint64_t after_len,
                       const uint8_t seed[32], uint64_t report[4]);

/* h-polynomial stage alone (7 NTTs + pointwise), device resident: a,b,c hold az,bz,cz zero-padded to
 * m scalars on entry; on return a[0 .. m-1) holds the h coefficients.  Exposed for parity tests. */
int32_t bzk_groth16_h_dev(bzk_ctx* ctx, void* a_dev, void* b_dev, void* c_dev, uint32_t log_m);

/* ---- a3 / a9: host-side MPN witness + R1CS generator (CPU, C++) --------------------------------
 * The part of the prover that bellman runs through `Circuit::synthesize`: restates
 * `impl Circuit for UpdateCircuit` (src/mpn/circuits/update_circuit.rs:49-494), the gadgets under
 * src/zk/groth16/gadgets/, the witness builder `update::update` (src/mpn/update.rs:8-299) over a
 * RAM-resident sparse account tree (src/zk/state/mod.rs semantics, MpnConfig::state_model
 * src/mpn/mod.rs:218-241) and the wallet's `create_mpn_transaction` (src/wallet/tx_builder.rs:287-306).
 * No GPU involved; the result feeds bzk_groth16_prove. */
typedef struct bzk_mpn bzk_mpn;   /* an MPN state: accounts, keys, mempool */
typedef struct bzk_r1cs bzk_r1cs; /* a synthesized circuit instance: assignment (+ matrices) */
int32_t bzk_mpn_create(uint32_t log4_tree, uint32_t log4_token_tree, bzk_mpn** out);
void bzk_mpn_destroy(bzk_mpn* w);
int32_t bzk_mpn_set_height(bzk_mpn* w, uint64_t height);
int32_t bzk_mpn_set_threads(bzk_mpn* w, int32_t n); /* worker threads of the witness generator (default: bzk_host_default_threads) */
/* the host generator's default thread count: the visible CPUs capped by the container's CPU quota (cgroup v2 cpu.max / v1 cfs quota);
 * BZK_HOST_THREADS=n overrides.  Read once per process. */
int32_t bzk_host_default_threads(void);
/* SURVEY 8f-3 ("replacing the per-tx KV walk in prepare_works", src/mpn/mod.rs:353-414): with a context set, the builders below and
 * bzk_mpn_make_work decide a batch from account DATA first and then re-hash its Merkle paths LEVEL BY LEVEL on the device - one
 * batched Poseidon launch per tree level over all transactions of the batch (~L + T + 2 launches instead of ~50 sequential host
 * hashes per transaction); the sibling inputs of those hashes are the transitions' Merkle proofs.  Transactions may share accounts.
 * Same transitions / MpnWork bytes as the host path.  ctx NULL: back to the host path.  The ctx must outlive its use here. */
int32_t bzk_mpn_set_device(bzk_mpn* w, bzk_ctx* ctx);
/* account `index` := keys from `JubJub::generate_keys(seed)` (src/crypto/jubjub/mod.rs:112-124), token
 * slot 0 = (token_id, balance); pub_xy_out (optional) receives address x|y */
int32_t bzk_mpn_add_account(bzk_mpn* w, uint64_t index, const uint8_t* seed, uint32_t seed_len, const uint8_t token_id[32],
                            uint64_t balance, uint8_t pub_xy_out[64]);
int32_t bzk_mpn_add_key(bzk_mpn* w, uint64_t index, const uint8_t* seed, uint32_t seed_len); /* key for a future account */
int32_t bzk_mpn_root(bzk_mpn* w, uint8_t root[32]);
/* queue a signed MpnTransaction src -> dst (nonce = sender nonce + 1 + already queued from that sender) */
int32_t bzk_mpn_push_tx(bzk_mpn* w, uint64_t src_index, uint64_t dst_index, const uint8_t token_id[32], uint64_t amount,
                        const uint8_t fee_token[32], uint64_t fee);
/* Mempool admission (src/blockchain/mempool.rs:258): verifies the n wire-form transactions (bzk_mpn_tx_verify_batch's input) and queues
 * those that verify, in input order, exactly as bzk_mpn_push_tx would have queued them.  With a context set (bzk_mpn_set_device) the
 * checks run on the device in one batch; without, on host threads (bzk_mpn_set_threads).  ok_out (n bytes, may be NULL), *accepted_out
 * (may be NULL).  Nothing is queued on BZK_E_ARG (bytes that are not n well-formed records: bzk_mpn_work_last_error). */
int32_t bzk_mpn_push_txs(bzk_mpn* w, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok_out, uint64_t* accepted_out);
/* Mempool admission of withdrawals (src/blockchain/mempool.rs:246-258, plus the calldata check the reference makes in its builder,
 * src/mpn/withdraw.rs:77): checks the n wire-form withdrawals (bzk_mpn_withdraw_verify_batch's input) and queues, in input order, those
 * whose payment.contract_id is the world's, whose withdraw_circuit_id is 0, whose token ids are residues' limbs and whose two verdict bits
 * are set.  They are queued with their payment bytes and the fingerprint derived from them, so bzk_mpn_make_work and the builders treat
 * them exactly like withdrawals queued by bzk_mpn_push_withdraw(..., fingerprint = NULL).  With a context set (bzk_mpn_set_device) the
 * checks run on the device; without, on host threads (bzk_mpn_set_threads).  ok_out (n bytes of 1 / 0, may be NULL), *accepted_out (may
 * be NULL).  Nothing is queued on BZK_E_ARG (bytes that are not n well-formed records, or a payment over 65 536 bytes:
 * bzk_mpn_work_last_error). */
int32_t bzk_mpn_push_withdraws(bzk_mpn* w, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok_out, uint64_t* accepted_out);
/* Mempool admission of deposits (src/blockchain/mempool.rs:241-258): checks the n wire-form deposits (bzk_mpn_deposit_verify_batch's input)
 * and queues, in input order, those whose payment.contract_id is the world's, whose deposit_circuit_id is 0, whose amount.token_id is a
 * residue's limbs and whose two verdict bits are set, each with its decompressed address, its amount and its payment bytes as received - so
 * bzk_mpn_make_work carries the payment unchanged and the builders (src/blockchain/ops/apply_deposit.rs:8) treat it like a deposit queued by
 * bzk_mpn_push_deposit.  With a context set the checks run on the device; without, on host threads.  ok_out (n bytes of 1 / 0, may be NULL),
 * *accepted_out (may be NULL).  Nothing is queued on BZK_E_ARG.  Fee token, minimum fee, nonce and balance rules stay with the node. */
int32_t bzk_mpn_push_deposits(bzk_mpn* w, const uint8_t* txs, uint64_t len, uint64_t n, uint8_t* ok_out, uint64_t* accepted_out);
/* applies up to 4^log4_batch queued txs (update::update), pads with UpdateTransition::null, synthesizes the
 * circuit.  Public inputs = [commitment, height, state, aux_data, next_state]. */
int32_t bzk_mpn_update_synthesize(bzk_mpn* w, uint32_t log4_batch, const uint8_t commitment[32], const uint8_t fee_token[32],
                                  int32_t record_matrices, bzk_r1cs** out);
/* Deposit / Withdraw (the other two `MpnWorkData` variants, src/mpn/mod.rs:243-248): DepositCircuit
 * (src/mpn/circuits/deposit_circuit.rs:47-293) with witness builder src/mpn/deposit.rs:11-233, WithdrawCircuit
 * (src/mpn/circuits/withdraw_circuit.rs:50-413) with src/mpn/withdraw.rs:10-259.  aux_data = root of the batch
 * tree (`reveal`, src/zk/groth16/gadgets/reveal/mod.rs:13-61).  `fingerprint` = ContractWithdraw::fingerprint()
 * (src/core/transaction.rs:204-211), taken as an opaque scalar: the L1 payment serialisation is out of scope. */
int32_t bzk_mpn_push_deposit(bzk_mpn* w, uint64_t key_index, const uint8_t token_id[32], uint64_t amount);
/* fingerprint NULL: the withdrawal carries a synthetic L1 payment and its fingerprint is derived from it as the wallet does
 * (src/wallet/tx_builder.rs:376-425); non-NULL: an opaque fingerprint (such a withdrawal cannot be put on the wire) */
int32_t bzk_mpn_push_withdraw(bzk_mpn* w, uint64_t account_index, const uint8_t token_id[32], uint64_t amount,
                              const uint8_t fee_token[32], uint64_t fee, const uint8_t fingerprint[32]);
/* a withdrawal signed elsewhere, queued as given: the key need not be one the world holds, the signature (r.x | r.y | s over
 * H2(fingerprint, nonce)) is only checked by the builder.  Opaque fingerprint, so no wire form (see above); a withdrawal received on the wire
 * goes through bzk_mpn_push_withdraws, which keeps its payment. */
int32_t bzk_mpn_push_withdraw_signed(bzk_mpn* w, const uint8_t pub_xy[64], uint32_t nonce, const uint8_t token_id[32], uint64_t amount,
                                     const uint8_t fee_token[32], uint64_t fee, const uint8_t fingerprint[32], const uint8_t sig[96]);
int32_t bzk_mpn_deposit_synthesize(bzk_mpn* w, uint32_t log4_batch, const uint8_t commitment[32], int32_t record_matrices, bzk_r1cs** out);
int32_t bzk_mpn_withdraw_synthesize(bzk_mpn* w, uint32_t log4_batch, const uint8_t commitment[32], int32_t record_matrices, bzk_r1cs** out);
/* all-disabled instances (kind 0 = deposit, 1 = withdraw), src/mpn/circuits/test.rs:151-229 */
int32_t bzk_mpn_circuit_empty(int32_t kind, uint32_t log4_tree, uint32_t log4_token_tree, uint32_t log4_batch,
                              const uint8_t commitment[32], uint64_t height, const uint8_t state[32], const uint8_t aux_data[32],
                              const uint8_t next_state[32], int32_t record_matrices, bzk_r1cs** out);
/* `MpnCircuit::empty(L, T, B)` with explicit public inputs (src/mpn/circuits/test.rs:117-132) */
int32_t bzk_mpn_update_empty(uint32_t log4_tree, uint32_t log4_token_tree, uint32_t log4_batch, const uint8_t commitment[32],
                             uint64_t height, const uint8_t state[32], const uint8_t aux_data[32], const uint8_t next_state[32],
                             const uint8_t fee_token[32], int32_t record_matrices, bzk_r1cs** out);
/* info: n_in, n_aux, n_constraints, nnz(A), nnz(B), nnz(C), first unsatisfied constraint + 1 (0 = satisfied),
 * accepted txs, rejected txs */
int32_t bzk_r1cs_info(const bzk_r1cs* r, uint64_t info[9]);
/* borrowed views: 0 z, 1 az, 2 bz, 3 cz, 4 a_density, 5 b_density, 6-8 val(A/B/C), 9-11 col(A/B/C) u32 flat
 * variable index, 12-14 row_ptr(A/B/C) u32 */
const void* bzk_r1cs_data(const bzk_r1cs* r, int32_t which, uint64_t* bytes);
void bzk_r1cs_free(bzk_r1cs* r);
/* Witness value traces on the device.  With bzk_mpn_set_defer(w, 1) a witness-only bzk_mpn_{update,deposit,withdraw}_synthesize does NOT
 * evaluate what hangs off Poseidon outputs - the Poseidon gadget's S-box / idle-lane variables (src/zk/groth16/gadgets/poseidon/mod.rs:8-95: two
 * thirds of a transition's constraints), the Merkle gadget's muxes (gadgets/merkle/mod.rs:21-78, common/mux.rs:7-47), the equality checks against
 * computed roots (common/number.rs:121-177) - but records a small program per circuit shape and, per transition, the values the host does know;
 * those slots of z / A.z / B.z / C.z are left untouched.  bzk_groth16_prove_r1cs (below, beside bzk_groth16_prove) uploads the arrays as they are
 * and runs the program on the device before anything reads them; bzk_r1cs_fill_host runs the SAME ops on the CPU for consumers of the complete
 * arrays (bzk_r1cs_data) - the result is byte-identical to a synthesis without deferral.  bzk_r1cs_info's satisfied-check covers the rows the host
 * wrote; the deferred rows are judged where they are computed (BZK_E_UNSAT from the prove call, info[9] after a host fill).
 *   defer_info: 0 deferred (1 / 0), 1 transitions, 2 ops of the program, 3 registers, 4 host-known values per transition, 5 dependency levels
 *               (a Merkle path is a chain of hashes), 6 / 7 variable / constraint slots per transition left to the device, 8 filled on the
 *               host (1 / 0), 9 flags of that fill (1 a deferred constraint does not hold, 2 a computed state differs from the builder's)
 * A second, opt-in level: bzk_mpn_set_defer_sig(w, 1) (or BZK_SYNTH_DEFER_SIG) defers the EdDSA gadget of every Update and Withdraw transition as well
 * (src/zk/groth16/gadgets/eddsa/mod.rs:77-280): its two 254-step double-and-add ladders and the four additions of its tail, 254 x (20 + 14) + 36 = 8 672
 * variables and as many constraints per signature, and its two final checks.  The hash of (R, pk, msg), both bit decompositions and the first bit's
 * muxes stay on the host.  The device computes the ladders' points (one inversion per ladder) before it fills their slots; a signature that does not
 * verify is reported like every deferred check (BZK_E_UNSAT, flags & 1).  It shows in defer_info's op, register, input and hole counts.  Deposit
 * has no signature gadget: its instance equals the BZK_SYNTH_DEFER one.  bzk_mpn_set_defer_sig implies bzk_mpn_set_defer; bzk_mpn_set_defer(w, 0)
 * turns both off, bzk_mpn_set_defer(w, 1) selects the first level alone - exactly the program it recorded before the second level existed. */
int32_t bzk_mpn_set_defer(bzk_mpn* w, int32_t on);
int32_t bzk_mpn_set_defer_sig(bzk_mpn* w, int32_t on);
int32_t bzk_r1cs_defer_info(const bzk_r1cs* r, uint64_t info[10]);
int32_t bzk_r1cs_fill_host(bzk_r1cs* r);
/* the schedule of the instance's program for the one-launch device kernel, checked on the host (no device needed): stages, segments, hash ops
 * covered, fill ops covered, largest segment (<= 64), violations (0: every op exactly once, in a stage its operands are ready for).  The signature
 * ladders of BZK_SYNTH_DEFER_SIG are not part of that schedule (they run in launches of their own, before and after it): neither counted nor missed */
int32_t bzk_r1cs_defer_schedule_info(const bzk_r1cs* r, uint64_t info[6]);
/* bzk_groth16_prove over an instance of the host generator (z / A.z / B.z / C.z are the instance's own pinned arrays), completing deferred
 * witness values on the device first.  BZK_E_UNSAT: a deferred constraint does not hold or a transition's computed state differs from the
 * witness builder's prediction (synthesize again without deferral for the exact first unsatisfied row). */
int32_t bzk_groth16_prove_r1cs(bzk_ctx* ctx, bzk_params* params, const bzk_r1cs* r, const uint8_t r_blind[32], const uint8_t s_blind[32],
                               uint8_t proof_out[387]);
/* Staging - the uploads and the deferred-value program in the witness PRODUCER's pipeline instead of the prover slot's.  bzk_r1cs_stage puts the
 * instance's z | A.z | B.z | C.z into HBM on `ctx`'s stream (a context of the producer's), runs the deferred-value program behind the uploads if the instance
 * has one, and returns at once; the instance's host arrays must stay alive until bzk_staged_wait (or a prove call on the handle) has returned.
 * bzk_groth16_prove_staged (any context of the same device) waits for that work in stream order and copies device to device instead of uploading; same proof
 * bytes, BZK_E_UNSAT as bzk_groth16_prove_r1cs.  bzk_staged_free hands the buffers back to the staging context (any thread; after the last prove call on the
 * handle has returned, before that context is destroyed). */
typedef struct bzk_staged bzk_staged;
int32_t bzk_r1cs_stage(bzk_ctx* ctx, const bzk_r1cs* r, bzk_staged** out);
int32_t bzk_staged_wait(bzk_staged* staged);
void bzk_staged_free(bzk_staged* staged);
/* read-back of one staged array (which: 0 z, 1 A.z, 2 B.z, 3 C.z) once the staging work has finished - i.e. what the DEVICE-side fill produced; *size_out = the
 * array's size, at most `cap` bytes are copied.  The counterpart of bzk_r1cs_fill_host + bzk_r1cs_data for the device executor: byte-identical to a synthesis
 * without deferral (what bellman's `ProvingAssignment` holds after `Circuit::synthesize`, src/mpn/circuits/update_circuit.rs:49-494). */
int32_t bzk_staged_read(const bzk_staged* staged, int32_t which, uint8_t* out, uint64_t cap, uint64_t* size_out);
int32_t bzk_groth16_prove_staged(bzk_ctx* ctx, bzk_params* params, const bzk_staged* staged, const uint8_t r_blind[32], const uint8_t s_blind[32],
                                 uint8_t proof_out[387]);
/* ---- proving from the witness alone: A.z, B.z, C.z on the device ------------------------------------------------------
 * bzk_groth16_prove wants <A_k, z>, <B_k, z>, <C_k, z> of every constraint from its caller.  The MPN generator produces them while it builds
 * the witness; a caller with a circuit of its own (the reference lets every contract bring its Groth16 key) holds a CRS from bzk_groth16_setup
 * and a witness, nothing else.  The circuit shape is fixed per CRS, so its matrices are resident data like the CRS: bzk_r1cs_mats_load once,
 * then bzk_groth16_prove_witness per proof - z is the only upload, the evaluations are written straight into the slot's h-stage buffers.
 * A handle is read-only after load: any number of prover slots of its device (one context + one slot per thread, as for bzk_params_slot) may
 * evaluate and prove from it at once.  Resident form: 8 bytes per non-zero (column + index into a dictionary of the distinct coefficients)
 * + 4 bytes per row and matrix; DESIGN.md 3.19. */
typedef struct bzk_r1cs_mats bzk_r1cs_mats;

/* A, B, C as bzk_groth16_setup takes them (flat variable indices, inputs then aux, rows including bellman's trailing
 * input_i * 0 = 0 constraints), made resident.  ctx = NULL: kept in host memory for the host-thread route.
 * A row may be empty, a column may repeat inside a row (the terms add), a stored coefficient may be zero.  BZK_E_ARG with bzk_last_error(ctx)
 * - bzk_last_error(NULL) on the ctx = NULL route - naming the matrix and the row, nothing allocated: the three n_rows differ; row_ptr[0] != 0 or
 * row_ptr descends; a column >= n_in + n_aux; a coefficient whose limbs are >= r; a NULL array with a non-zero count; n_in = 0. */
int32_t bzk_r1cs_mats_load(bzk_ctx* ctx, const bzk_csr* A, const bzk_csr* B, const bzk_csr* C,
                           uint32_t n_in, uint32_t n_aux, bzk_r1cs_mats** out);
/* the same from views 6 - 14 of an instance synthesized with record_matrices */
int32_t bzk_r1cs_mats_from_r1cs(bzk_ctx* ctx, const bzk_r1cs* r, bzk_r1cs_mats** out);
void    bzk_r1cs_mats_free(bzk_ctx* ctx, bzk_r1cs_mats* m);
/* info: n_rows, n_vars, nnz(A), nnz(B), nnz(C), distinct coefficients, resident bytes, 0 */
int32_t bzk_r1cs_mats_info(const bzk_r1cs_mats* m, uint64_t info[8]);

/* az / bz / cz: n_rows x 32 B each, any of them may be NULL: canonical Montgomery scalars, byte for byte what bzk_r1cs_data views 1 - 3 hold.
 * z is taken as canonical; an entry whose limbs are >= r is not refused and no read leaves the arrays whatever it evaluates to.
 * first_unsat (may be NULL): index of the first row with az * bz != cz, or -1.
 * ctx = NULL: the same per-row function on host threads (a handle loaded with ctx = NULL; a device-resident one is refused there, and a
 * host one here).  BZK_E_ARG, nothing launched: n_vars != n_in + n_aux of the handle, a NULL z, a handle of the other kind or of another device. */
int32_t bzk_r1cs_eval(bzk_ctx* ctx, const bzk_r1cs_mats* m, const uint8_t* z, uint64_t n_vars,
                      uint8_t* az, uint8_t* bz, uint8_t* cz, int64_t* first_unsat);
/* device pointers, enqueued on the context's stream.  Each output holds pad_rows >= n_rows scalars,
 * rows n_rows .. pad_rows are written as zero (the h stage's padding).  BZK_E_ARG as above, and for pad_rows < n_rows. */
int32_t bzk_r1cs_eval_dev(bzk_ctx* ctx, const bzk_r1cs_mats* m, const void* z_dev, uint64_t n_vars,
                          void* az_dev, void* bz_dev, void* cz_dev, uint64_t pad_rows);

#define BZK_PROVE_CHECK_SAT 1u  /* BZK_E_UNSAT, bzk_last_error naming the first unsatisfied row, nothing written to proof_out */
/* bzk_groth16_prove from z alone: the 387 bytes bzk_groth16_prove gives for the same z, r, s and the evaluations of z.  BZK_E_ARG, nothing
 * launched, the context proves normally afterwards: n_vars != n_in + n_aux of the handle or of the params, n_rows > 2^log_m, a NULL z, a handle
 * in host memory or of another device.  Without BZK_PROVE_CHECK_SAT an unsatisfied witness yields an (invalid) proof, as bzk_groth16_prove does;
 * with it, one product per row on the device decides, and the smallest failing index is reported. */
int32_t bzk_groth16_prove_witness(bzk_ctx* ctx, bzk_params* params, const bzk_r1cs_mats* m, const uint8_t* z, uint64_t n_vars,
                                  const uint8_t r[32], const uint8_t s[32], uint32_t flags, uint8_t proof_out[387]);
/* CPU mirrors of `ZkHasher::hash`, `hash_to_scalar`'s SHA3 and `JubJub::{generate_keys, sign, verify}` */
/* ---- f-2: the proving worker's wire format ---------------------------------------------------------------------------
 * `MpnWork` (src/mpn/mod.rs:263-270) as `GET /bincode/mpn/work` delivers it (src/node/mod.rs:393-398,
 * src/client/messages.rs:368-376) and `ZkProof` (src/zk/mod.rs:646-651) as `POST /bincode/mpn/solution` takes it, both
 * bincode 1.3.3 with default options.  Layouts: bazuka_amd/csrc/host_bincode.h.  A Rust host that already holds an
 * `MpnWork` passes `bincode::serialize(&work)`; the worker loop of bazuka_amd/worker.py passes the HTTP body. */
#define BZK_WORK_SIG_LEN_PREFIXED 1u /* ed25519 signatures inside L1 payments carry a u64 length (ed25519 < 1.3) */
typedef struct bzk_mpn_work bzk_mpn_work;
/* decodes ONE MpnWork from the front of `bytes`; *consumed = its encoded length (a response holds several) */
int32_t bzk_mpn_work_decode(const uint8_t* bytes, uint64_t len, uint32_t flags, bzk_mpn_work** out, uint64_t* consumed);
const char* bzk_mpn_work_last_error(void); /* why the last decode on this thread failed */
void bzk_mpn_work_free(bzk_mpn_work* work);
/* info = kind (0 deposit, 1 withdraw, 2 update), log4_tree, log4_token_tree, log4 batch size of that kind, transitions on
 * the wire, height, reward, new_root.state_size, mpn_num_{update,deposit,withdraw}_batches, this work's VK byte length */
int32_t bzk_mpn_work_info(const bzk_mpn_work* work, uint64_t info[12]);
/* out = state | aux_data | next_state | new_root.state_hash | mpn_contract_id, 32 bytes each */
int32_t bzk_mpn_work_scalars(const bzk_mpn_work* work, uint8_t out[160]);
/* bincode(Groth16VerifyingKey) (src/zk/groth16/mod.rs:22-31); which = -1: `MpnWork::vk()`, 0/1/2: deposit/withdraw/update */
int32_t bzk_mpn_work_vk(const bzk_mpn_work* work, int32_t which, uint8_t* out, uint64_t cap, uint64_t* len);
/* ZkScalar::new(sha3_256(bincode((prover, reward)))) - the commitment `MpnWork::verify` binds a solution to
 * (src/mpn/mod.rs:281-295); prover_pub = the worker's 32-byte ed25519 address */
int32_t bzk_mpn_work_commitment(const bzk_mpn_work* work, const uint8_t prover_pub[32], uint8_t out[32]);
/* `MpnWork::verify(prover, proof)` (src/mpn/mod.rs:281-295) on the host: 1 accepted / 0 refused / negative bad arguments */
int32_t bzk_mpn_work_verify(const bzk_mpn_work* work, const uint8_t prover_pub[32], const uint8_t proof[387]);
/* the circuit instance to prove: transitions padded with null ones to 4^batch; fee_token NULL = Ziesha; threads 0 = all;
 * record_matrices: 0 witness only, 1 with the CSR matrices (setup), BZK_SYNTH_DEFER witness only with the hash-dependent values of the
 * work's transitions left to the device (see bzk_mpn_set_defer; all three kinds), BZK_SYNTH_DEFER_SIG the same with the signature gadget deferred too
 * (bzk_mpn_set_defer_sig; 4, not 3: every value but 0, 1 and 2 was refused with BZK_E_ARG before, and 3 stays refused) */
#define BZK_SYNTH_DEFER 2
#define BZK_SYNTH_DEFER_SIG 4
int32_t bzk_mpn_work_synthesize(const bzk_mpn_work* work, const uint8_t prover_pub[32], const uint8_t fee_token[32],
                                int32_t threads, int32_t record_matrices, bzk_r1cs** out);
int32_t bzk_mpn_work_encode(const bzk_mpn_work* work, uint8_t* out, uint64_t cap, uint64_t* len); /* out NULL: size query */
/* validator side (`prepare_works`, src/mpn/mod.rs:298-424): one work of the given kind from the world's queued
 * transactions; the world advances to the work's next_state */
typedef struct {
    uint8_t log4_deposit_batch, log4_withdraw_batch, log4_update_batch;
    uint64_t num_update_batches, num_deposit_batches, num_withdraw_batches;
    const uint8_t* deposit_vk;  uint64_t deposit_vk_len;  /* bincode(Groth16VerifyingKey) */
    const uint8_t* withdraw_vk; uint64_t withdraw_vk_len;
    const uint8_t* update_vk;   uint64_t update_vk_len;
    uint64_t new_root_state_size; /* ZkCompressedState::state_size: bookkeeping of the node's KV store, passed through */
} bzk_mpn_work_config;
int32_t bzk_mpn_make_work(bzk_mpn* w, int32_t kind, const bzk_mpn_work_config* cfg, uint64_t reward, bzk_mpn_work** out);
int32_t bzk_zkproof_encode(const uint8_t proof[387], uint8_t out[391]); /* ZkProof::Groth16(Box<Groth16Proof>) */
int32_t bzk_zkproof_decode(const uint8_t* in, uint64_t len, uint8_t proof[387]);

int32_t bzk_host_poseidon(const uint8_t* in, uint32_t arity, uint8_t out[32]);
int32_t bzk_host_scalar_new(const uint8_t* le_bytes, uint32_t len, uint8_t out[32]); /* ZkScalar::new: LE integer mod r; len <= 64 */
int32_t bzk_host_sha3_256(const uint8_t* in, uint64_t len, uint8_t out[32]);
int32_t bzk_host_jubjub_keys(const uint8_t* seed, uint32_t len, uint8_t out[128]); /* pub.x|pub.y|randomness|scalar */
int32_t bzk_host_jubjub_sign(const uint8_t key[128], const uint8_t msg[32], uint8_t sig_out[96]); /* r.x|r.y|s */
int32_t bzk_host_jubjub_verify(const uint8_t pub_xy[64], const uint8_t msg[32], const uint8_t sig[96]); /* 1 / 0 */
/* PointCompressed::decompress (src/crypto/jubjub/curve.rs:78-88) on the host.  x: 32 B Montgomery, odd: 0 / 1.  Returns 1 / 0; 0 (and
 * xy_out = zeros) where the reference panics (no square root) or x is not a residue's limbs.  Negative on bad arguments. */
int32_t bzk_host_jubjub_decompress(const uint8_t x[32], int32_t odd, uint8_t xy_out[64]);
int32_t bzk_host_sha512(const uint8_t* in, uint64_t len, uint8_t out[64]);
/* the verdict of bzk_ed25519_verify_batch for one signature, on the host */
int32_t bzk_host_ed25519_verify(const uint8_t pk[32], const uint8_t* msg, uint64_t len, const uint8_t sig[64]);  /* 1 / 0 */
/* one row of bzk_ed25519_keys_batch / bzk_ed25519_sign_batch on the host: keys_out / keys = secret | public, sig_out = R | s */
int32_t bzk_host_ed25519_keys(const uint8_t* seed, uint64_t len, uint8_t keys_out[64]);
int32_t bzk_host_ed25519_sign(const uint8_t keys[64], const uint8_t* msg, uint64_t len, uint8_t sig_out[64]);

/* ---- static-base tables (the Groth16 CRS queries are fixed point sets) -------------------------------------------
 * build: tab[w][i] = 2^(c w) * base_i for every window, kept in HBM (W x the base memory, internal limb form).  With a
 * table every window feeds ONE bucket set: the bucket reduction shrinks from W windows to one and no host-side Horner
 * remains.  Same result bytes as bzk_msm_*_dev on the same inputs.  n scalars (n <= table size) use bases [0, n). */
typedef struct bzk_msm_table bzk_msm_table;
int32_t bzk_msm_g1_table_build(bzk_ctx* ctx, const void* bases_dev, uint64_t n, bzk_msm_table** out);
int32_t bzk_msm_g2_table_build(bzk_ctx* ctx, const void* bases_dev, uint64_t n, bzk_msm_table** out);
/* full table with an explicit window size c (4 .. 22): every window shares one set of 2^(c-1) buckets, so c can grow to ~log2 n -
 * fewer windows, i.e. fewer additions per point: 2^20 points, c = 20: 13 levels (1.5 GB), 3.93 ms against 4.32 ms for the per-call
 * pipeline on raw bases (profiles/r02_run17_static_tables.txt).  What bzk_groth16_prove uses for the (static) h query. */
int32_t bzk_msm_g1_table_build_c(bzk_ctx* ctx, const void* bases_dev, uint64_t n, uint32_t c, bzk_msm_table** out);
/* folded table: `levels` L < W levels tab[j][i] = 2^(c wpl j) * base_i, wpl = ceil(W / L): windows j * wpl + w' share bucket
 * set w' - the same number of point additions, 1 / L of the buckets to reduce, L x the base memory (levels = 0 or >= W: the
 * full table).  For a folded table the `windows` range of *_table_windows_dev selects bucket sets [w_begin, w_end) of the
 * bzk_msm_table_window_count() = wpl sets; the partial results still add up to the full MSM (bzk_g1_sum / bzk_g2_sum). */
int32_t bzk_msm_g1_table_build_levels(bzk_ctx* ctx, const void* bases_dev, uint64_t n, uint32_t levels, bzk_msm_table** out);
int32_t bzk_msm_g2_table_build_levels(bzk_ctx* ctx, const void* bases_dev, uint64_t n, uint32_t levels, bzk_msm_table** out);
uint32_t bzk_msm_table_levels(const bzk_msm_table* table);
int32_t bzk_msm_g1_table_run_dev(bzk_ctx* ctx, const bzk_msm_table* table, const void* scalars_dev, uint64_t n, uint32_t flags, uint8_t out[97]);
int32_t bzk_msm_g2_table_run_dev(bzk_ctx* ctx, const bzk_msm_table* table, const void* scalars_dev, uint64_t n, uint32_t flags, uint8_t out[193]);
int32_t bzk_msm_g1_table_windows_dev(bzk_ctx* ctx, const bzk_msm_table* table, const void* scalars_dev, uint64_t n, uint32_t flags,
                                     uint32_t w_begin, uint32_t w_end, uint8_t out[97]);
int32_t bzk_msm_g2_table_windows_dev(bzk_ctx* ctx, const bzk_msm_table* table, const void* scalars_dev, uint64_t n, uint32_t flags,
                                     uint32_t w_begin, uint32_t w_end, uint8_t out[193]);
uint32_t bzk_msm_table_window_count(const bzk_msm_table* table);
void bzk_msm_table_free(bzk_ctx* ctx, bzk_msm_table* table);

/* ---- resident base sets --------------------------------------------------------------------------------------------
 * A Groth16 CRS query is a STATIC point set (bellman `Parameters`: h, l, a, b_g1, b_g2): load converts it once into the
 * library's internal limb form (G1 112 B, G2 224 B per point) and keeps it in HBM; every later MSM over it - and every
 * rank of a window-sharded MSM - gathers from the resident set and converts nothing per call.  Same result bytes as
 * bzk_msm_*_dev on the raw bases.  n scalars (n <= set size) use bases [0, n).  A set is read-only after load and may be
 * shared by any number of contexts of the same device. */
typedef struct bzk_msm_bases bzk_msm_bases;
int32_t bzk_msm_g1_bases_load_dev(bzk_ctx* ctx, const void* bases_dev, uint64_t n, bzk_msm_bases** out);
int32_t bzk_msm_g2_bases_load_dev(bzk_ctx* ctx, const void* bases_dev, uint64_t n, bzk_msm_bases** out);
void bzk_msm_bases_free(bzk_ctx* ctx, bzk_msm_bases* bases);
uint64_t bzk_msm_bases_size(const bzk_msm_bases* bases);
/* What a load decided: *forms = 1 (the set alone) or the number of arrays held - the set plus its endomorphism images X^m P (G1: 2,
 * G2: 4), which whole-MSM calls flagged BZK_F_THROUGHPUT use (fewer bucket sets, same additions, same result).  The images are built
 * at load unless no call could use them (BZK_MSM_ENDO_G1 / _G2 = 0, BZK_MSM_NO_ENDO = 1, device groups) or they do not fit beside an
 * 8 GiB reserve; *device_bytes = HBM held by the set, its window table (below) included. */
int32_t bzk_msm_bases_info(const bzk_msm_bases* bases, uint64_t* n, int32_t* forms, uint64_t* device_bytes);
/* The window table of a resident G1 set.  A load of 2^19 < n <= 2^20 points also builds the full static table 2^(20 w) P_i (13 levels x 112 B x n: 1.5 GB
 * at 2^20 points) when it fits beside the same 8 GiB reserve, and a whole stand-alone call over the set - bzk_msm_g1_bases_run_dev without
 * BZK_F_THROUGHPUT / BZK_F_DEDUP, on a context with no forced window (BZK_MSM_C) and no BZK_MSM_SPLIT* setting - runs from it: 13 additions per
 * point instead of 16, one bucket set, the same result bytes.  Every other call over the set is unchanged.  Env, read when a context is
 * created: BZK_MSM_BASES_TABLE=0 never builds a table, =1 builds one for every G1 set it fits; BZK_MSM_BASES_TABLE_C = 11 .. 20 sets the table's window.
 * The sets that bzk_groth16_prove and the device groups load for themselves never carry one.  *c = the table's window, *levels = its
 * levels, *table_bytes = 112 x levels x n; all 0 for a set without a table. */
int32_t bzk_msm_bases_table_info(const bzk_msm_bases* bases, uint32_t* c, uint32_t* levels, uint64_t* table_bytes);
int32_t bzk_msm_g1_bases_run_dev(bzk_ctx* ctx, const bzk_msm_bases* bases, const void* scalars_dev, uint64_t n, uint32_t flags, uint8_t out[97]);
int32_t bzk_msm_g2_bases_run_dev(bzk_ctx* ctx, const bzk_msm_bases* bases, const void* scalars_dev, uint64_t n, uint32_t flags, uint8_t out[193]);
int32_t bzk_msm_g1_bases_windows_dev(bzk_ctx* ctx, const bzk_msm_bases* bases, const void* scalars_dev, uint64_t n, uint32_t flags,
                                     uint32_t w_begin, uint32_t w_end, uint8_t out[97]);
int32_t bzk_msm_g2_bases_windows_dev(bzk_ctx* ctx, const bzk_msm_bases* bases, const void* scalars_dev, uint64_t n, uint32_t flags,
                                     uint32_t w_begin, uint32_t w_end, uint8_t out[193]);

/* ---- row (e): multi-GPU ------------------------------------------------------------------------------------------------
 * A device GROUP behind the boundary: a Rust prover drives 1..8 MI355X of a node through these entry points alone (no
 * torch.distributed, no Python).  SURVEY.md 8b proposed `bzk_ctx_create(device_ids, n)`; the group is its own handle so that
 * the single-device ctx keeps its one-stream, one-thread contract.
 *   MSM    : sharded by SCALAR-WINDOW RANGE over the group (north star): rank r computes windows [W r / world, W (r + 1) / world)
 *            over all points from a resident base set replicated at load time; ONE all-gather of the W window sums (3 - 6 KB
 *            for the whole group; RCCL cannot add curve points, so gather + combine), then the Horner combine over the W windows
 *            on the host, as in the single-GPU call.  Same 97 / 193 result bytes as bzk_msm_g*_dev.
 *   proofs : replicas (the reference's own split of a block's proofs over provers, src/mpn/mod.rs:79-107): a pool of prover slots
 *            on every device takes proofs from one queue (submit / wait), CRS shared per device.
 * Deployments: bzk_mg_create - ONE process drives n devices (one persistent host thread each; device ids may repeat, e.g. for a
 * rehearsal on a one-GPU box); bzk_mg_create_rank - one process PER GPU (torchrun style): rank 0 draws bzk_mg_unique_id() and
 * the host hands the 128 bytes to the other ranks by its own means, every rank then calls bzk_mg_create_rank and later the same
 * bzk_mg_msm_* call with its own device pointers; every rank receives the result.
 * Exchange: BZK_MG_X_RCCL = ncclAllGather(uint8) over xGMI (librccl is loaded at run time); BZK_MG_X_HOST = pinned host memory
 * (one process) or a POSIX shared-memory segment (process per GPU, single node) - the only transport for ranks that SHARE a
 * device; BZK_MG_X_PEER = hipMemcpyPeerAsync into device 0 (one process).  BZK_MG_X_AUTO = RCCL when the group spans distinct
 * devices and librccl loads, else HOST.  One collective call at a time per group; bzk_mg_ctx(i) exposes the i-th local context
 * (allocation, uploads, profiling) and must not be used concurrently with a group call. */
#define BZK_MG_UID_BYTES 128
#define BZK_MG_X_AUTO 0u
#define BZK_MG_X_HOST 1u
#define BZK_MG_X_PEER 2u
#define BZK_MG_X_RCCL 3u
typedef struct bzk_mg bzk_mg;
typedef struct bzk_mg_bases bzk_mg_bases;
int32_t bzk_mg_unique_id(uint8_t uid[BZK_MG_UID_BYTES]);
/* what THIS process could contribute to a group on `device_id`, without creating anything that a peer would wait for: a bit mask,
 * bit 0 = the device exists and is a gfx950, bit 1 = librccl is loadable with every entry point the RCCL exchange needs.  A
 * process-per-GPU host publishes the answer of every rank (by its own means) BEFORE calling bzk_mg_create_rank with BZK_MG_X_RCCL:
 * ncclCommInitRank blocks until all ranks arrive, so a rank that cannot take part must be known beforehand.  Negative: BZK_E_*. */
int32_t bzk_mg_probe(int32_t device_id);
int32_t bzk_mg_create(const int32_t* device_ids, int32_t n_devices, uint32_t exchange, bzk_mg** out);
int32_t bzk_mg_create_rank(int32_t device_id, int32_t rank, int32_t world, const uint8_t uid[BZK_MG_UID_BYTES], uint32_t exchange, bzk_mg** out);
void bzk_mg_destroy(bzk_mg* mg);
int32_t bzk_mg_world(const bzk_mg* mg);      /* ranks of the group */
int32_t bzk_mg_local(const bzk_mg* mg);      /* devices this process drives */
int32_t bzk_mg_rank(const bzk_mg* mg);       /* rank of local device 0 */
uint32_t bzk_mg_exchange(const bzk_mg* mg);  /* the transport in use (BZK_MG_X_*) */
bzk_ctx* bzk_mg_ctx(bzk_mg* mg, int32_t local_index);
/* Where the window-sharded calls of this rank spent their time (cumulative; reset != 0 clears the per-call sums afterwards):
 *   out[0] calls   out[1] local stage, ms (this rank's windows, device side, local device 0)   out[2] exchange, ms (device side: the
 *   all-gather / peer copies and the read-back queued behind the local stage)   out[3] waiting for the other ranks, ms (host side:
 *   the shared-memory transport's barrier)   out[4] host combine (Horner), ms   out[5] group creation, s   out[6] of which the
 *   communicator (ncclCommInitRank / ncclCommInitAll), s   out[7] reserved.  A slow rank shows up as exchange / waiting time of the others. */
int32_t bzk_mg_stats(bzk_mg* mg, int32_t reset, double out[8]);
const char* bzk_mg_last_error(bzk_mg* mg);
/* replicate a static base set on every local device (host pointer: uploaded + converted per device; _dev: one device pointer
 * per local device, raw affine) */
int32_t bzk_mg_bases_g1_load(bzk_mg* mg, const uint8_t* bases_host, uint64_t n, bzk_mg_bases** out);
int32_t bzk_mg_bases_g2_load(bzk_mg* mg, const uint8_t* bases_host, uint64_t n, bzk_mg_bases** out);
int32_t bzk_mg_bases_g1_load_dev(bzk_mg* mg, const void* const* bases_dev, uint64_t n, bzk_mg_bases** out);
int32_t bzk_mg_bases_g2_load_dev(bzk_mg* mg, const void* const* bases_dev, uint64_t n, bzk_mg_bases** out);
void bzk_mg_bases_free(bzk_mg* mg, bzk_mg_bases* bases);
/* scalars: one host vector (broadcast to the local devices), or one DEVICE pointer per local device holding the same n scalars */
int32_t bzk_mg_msm_g1(bzk_mg* mg, const bzk_mg_bases* bases, const uint8_t* scalars, uint64_t n, uint32_t flags, uint8_t out[97]);
int32_t bzk_mg_msm_g2(bzk_mg* mg, const bzk_mg_bases* bases, const uint8_t* scalars, uint64_t n, uint32_t flags, uint8_t out[193]);
int32_t bzk_mg_msm_g1_dev(bzk_mg* mg, const bzk_mg_bases* bases, const void* const* scalars_dev, uint64_t n, uint32_t flags, uint8_t out[97]);
int32_t bzk_mg_msm_g2_dev(bzk_mg* mg, const bzk_mg_bases* bases, const void* const* scalars_dev, uint64_t n, uint32_t flags, uint8_t out[193]);

/* proof pool over the group's local devices: `slots_per_device` prover slots (context + lanes + scratch each) per device over ONE
 * CRS upload per device; one host thread per slot takes proofs from a common queue (whichever slot is free next).  The assignment
 * arrays and proof_out must stay valid until the ticket has been waited for; wait returns that proof's status. */
typedef struct bzk_mg_params bzk_mg_params;
int32_t bzk_mg_params_load(bzk_mg* mg, const bzk_params_desc* desc, uint32_t slots_per_device, bzk_mg_params** out);
void bzk_mg_params_free(bzk_mg* mg, bzk_mg_params* params);
uint32_t bzk_mg_params_slots(const bzk_mg_params* params);
int32_t bzk_mg_params_stats(bzk_mg_params* params, uint64_t* proofs_per_slot, uint32_t cap);
int32_t bzk_mg_prove_submit(bzk_mg* mg, bzk_mg_params* params, const bzk_assignment* asg, const uint8_t r[32], const uint8_t s[32],
                            uint8_t proof_out[387], uint64_t* ticket);
int32_t bzk_mg_prove_wait(bzk_mg* mg, bzk_mg_params* params, uint64_t ticket);
int32_t bzk_mg_prove(bzk_mg* mg, bzk_mg_params* params, const bzk_assignment* asg, const uint8_t r[32], const uint8_t s[32],
                     uint8_t proof_out[387]);

/* synthetic-input helpers (device side, for benches and tests): base_i = k_i * G with
 * k_i = SplitMix64(seed + 0x632BE59BD9B4E019 * (start+i)).next() | 1 ; raw affine out */
int32_t bzk_g1_synth_bases_dev(bzk_ctx* ctx, uint64_t seed, uint64_t start, uint64_t n, void* out_dev);
int32_t bzk_g2_synth_bases_dev(bzk_ctx* ctx, uint64_t seed, uint64_t start, uint64_t n, void* out_dev);

#ifdef __cplusplus
}
#endif
#endif /* BZK_H */
