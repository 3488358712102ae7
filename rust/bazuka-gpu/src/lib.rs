//! bazuka-gpu: the Rust side of the drop-in boundary - Bazuka's own types over `libbzk.so` (MI355X).
//!
//! **UNVERIFIED BY COMPILATION.**  The image that builds and tests libbzk has no rustc / cargo; this file is shipped as source.
//! What IS checked mechanically (tests/test_rust_shim_cpu.py): every `sys::` symbol used here exists in `bzk-sys`, whose
//! declarations are generated from `include/bzk.h` and compared with it on every test run; argument counts of each call; the
//! reference signatures quoted in the doc comments below.  Everything else is for a maintainer with a Rust toolchain to compile.
//!
//! Each public item names the reference interface it stands beside (paths relative to ziesha-network/bazuka v0.19.20):
//!   * `GpuPoseidonHasher`      - `impl ZkHasher` (src/zk/mod.rs:152-155, 496-511) + the BULK path `hash_batch`
//!   * `Gpu::jubjub_verify_batch` - `JubJub::<ZkHasher>::verify` (src/crypto/jubjub/mod.rs:151-167) for many signatures at once
//!   * `Gpu::jubjub_keys_batch` / `Gpu::jubjub_sign_batch` - `JubJub::generate_keys` and `JubJub::sign` (src/crypto/jubjub/mod.rs:112-150) for many
//!                                seeds / (key, message) pairs at once; `Gpu::mpn_txs_sign` - the signing step of
//!                                `TxBuilder::create_mpn_transaction` (src/wallet/tx_builder.rs:287-306) for many transactions at once;
//!                                `Gpu::mpn_withdraws_sign` - the signature and calldata of `TxBuilder::withdraw_mpn` (:376-425) for many withdrawals
//!   * `Gpu::ed25519_keys_batch` / `Gpu::ed25519_sign_batch` - `Ed25519::generate_keys` and `Ed25519::sign` (src/crypto/ed25519.rs:70-80) for many
//!                                seeds / (keypair, message) pairs at once; `Gpu::mpn_deposits_sign` / `Gpu::l1_txs_sign` - `TxBuilder::sign_deposit`
//!                                and `TxBuilder::sign_tx` (src/wallet/tx_builder.rs:63-70) for many records at once
//!   * `Gpu::mpn_tx_verify_batch` - `MpnTransaction::verify_signature` (src/zk/mod.rs:610-627) for many wire-form transactions at once
//!   * `Gpu::mpn_withdraw_verify_batch` - `MpnWithdraw::verify_signature` and `verify_calldata` (src/core/transaction.rs:177-189) for many
//!                                wire-form withdrawals at once, with `payment.fingerprint()` (:204-211, a SHA3-256) taken on the device
//!   * `Gpu::sha3_256_batch`    - `hash_to_scalar` (src/zk/mod.rs:218-220) for many messages at once
//!   * `Gpu::mpn_deposit_verify_batch` - `ContractDeposit::verify_signature` (src/core/transaction.rs:192-202) for many wire-form deposits at
//!                                once, and whether each `mpn_address` decompresses
//!   * `Gpu::ed25519_verify_batch` - `Ed25519::verify` (src/crypto/ed25519.rs:81-83) for many (key, message, signature) at once
//!   * `Gpu::sha512_batch`      - SHA-512 of many messages at once
//!   * `Gpu::l1_tx_verify_batch` - `Transaction::verify_signature` and `Transaction::hash` (src/core/transaction.rs:383-397) for many L1
//!                                transactions at once, the signed form hashed in place on the device
//!   * `Gpu::sha3_merkle_root`  - `MerkleTree::<Sha3Hasher>::new(leaves).root()` (src/crypto/merkle.rs)
//!   * `Gpu::block_bodies_check` - the body checks of src/blockchain/ops/apply_block.rs:47 and :88 for many blocks in one call
//!   * `Gpu::check_contract_updates` - what `update_contract` (src/blockchain/ops/apply_tx/update_contract/mod.rs:28-116) computes and verifies
//!                                per `ContractUpdate`: commitment, aux data, deposit signatures, proof - for many transactions of one contract
//!   * `contract_update_spans`  - where the `ContractUpdate`s of one contract lie in serialized transactions (host only)
//!   * `groth16_prove`          - beside `groth16_verify` (src/zk/groth16/mod.rs:67-75), same argument order
//!   * `groth16_verify_batch`   - `groth16_verify` for n proofs of one key: update_contract/mod.rs:100 and `MpnWork::verify` (src/mpn/mod.rs:281-295)
//!   * `Gpu::groth16_verify_batch_keys` - the same for proofs of several keys (a block's Deposit, Withdraw and Update proofs) in one set of launches
//!   * `compress`               - `ZkStateModel::compress::<H>(&data)` (src/zk/mod.rs:392-399)
//!   * `DeviceStateManager`     - `KvStoreStateManager::{update_contract, root, get_data, prove}` (src/zk/state/mod.rs:218-438) for one
//!                                contract with the values resident on the GPU
//!   * `prove_work`             - an `MpnWork` (src/mpn/mod.rs:263-270) -> the `ZkProof` that `MpnWork::verify` (:281-295) accepts
//!   * `DeviceGroup`            - 1..8 GPUs of a node: window-sharded MSM + a proof pool (no torch, no Python)
//!
//! Process-level runtime settings a PROVING host should make before its first call into libbzk (they are read when the HIP runtime initialises; the
//! library cannot make them for a process that already did): `GPU_MAX_HW_QUEUES=16` (a prover keeps 4 slots x 4 streams busy) and
//! `AMD_DIRECT_DISPATCH=0` (launches through the runtime's worker threads: the prover side costs the host 0.0084 instead of 0.0202 CPU-s per proof,
//! four slots prove 4 % more per second under a CPU quota; a caller of lone MSMs keeps the default - 2 % faster for it).  `std::env::set_var` at
//! the top of `main`, as bazuka_amd/csrc/worker_main.cpp does with `setenv`; INTEGRATION.md, environment table.
//!
//! Layout assumptions (already relied upon by the reference's own `transmute`s, src/zk/groth16/mod.rs:7-17): `ZkScalar` is
//! `[u64; 4]` little-endian Montgomery limbs; bincode 1.3 with default options; `Groth16Proof` = 97 + 193 + 97 bytes under bincode.
use bazuka::core::{Address, Block, ContractId, ContractUpdate, MpnDeposit, MpnWithdraw, Transaction};
use bazuka::crypto::jubjub::{PointAffine, PrivateKey, PublicKey, Signature};
use bazuka::mpn::MpnWork;
use bazuka::zk::groth16::Groth16Proof;
use bazuka::zk::{
    MpnTransaction, StateManagerError, ZkCompressedState, ZkDataLocator, ZkDataPairs, ZkDeltaPairs, ZkHasher, ZkLocatorError, ZkProof, ZkScalar,
    ZkContract, ZkStateModel, ZkVerifierKey,
};
use bzk_sys as sys;
use std::ffi::CStr;
use std::ptr;
use std::sync::{Mutex, OnceLock};

#[derive(thiserror::Error, Debug)]
pub enum GpuError {
    #[error("libbzk: {0} ({1})")]
    Status(i32, String),
    #[error("bincode: {0}")]
    Bincode(#[from] bincode::Error),
}

fn check(ctx: *mut sys::bzk_ctx, st: i32) -> Result<(), GpuError> {
    if st == sys::BZK_OK {
        return Ok(());
    }
    let detail = unsafe {
        let p = if ctx.is_null() { sys::bzk_strerror(st) } else { sys::bzk_last_error(ctx) };
        CStr::from_ptr(p).to_string_lossy().into_owned()
    };
    Err(GpuError::Status(st, detail))
}

fn scalars_ptr(v: &[ZkScalar]) -> *const u8 {
    v.as_ptr() as *const u8
}

/// One GPU + one HIP stream.  There is no CPU fallback: construction fails without a gfx950 device.
pub struct Gpu(*mut sys::bzk_ctx);
unsafe impl Send for Gpu {}

impl Gpu {
    pub fn new(device: i32) -> Result<Self, GpuError> {
        let mut h = ptr::null_mut();
        check(ptr::null_mut(), unsafe { sys::bzk_ctx_create(device, ptr::null_mut(), &mut h) })?;
        Ok(Gpu(h))
    }

    /// Bulk `ZkHasher::hash`: out[i] = poseidon(vals[i * arity .. (i + 1) * arity])  (src/zk/poseidon/mod.rs:24-84)
    pub fn hash_batch(&self, vals: &[ZkScalar], arity: usize) -> Result<Vec<ZkScalar>, GpuError> {
        assert!(arity >= 1 && arity <= 16 && vals.len() % arity == 0);
        let n = vals.len() / arity;
        let mut out = vec![ZkScalar::default(); n];
        check(self.0, unsafe { sys::bzk_poseidon_batch(self.0, scalars_ptr(vals), arity as u32, n as u64, out.as_mut_ptr() as *mut u8) })?;
        Ok(out)
    }

    /// Bulk `JubJub::<PoseidonHasher>::verify(pk, msg, sig)` (src/crypto/jubjub/mod.rs:151-167): one verdict per (key, message, signature).
    /// The keys go to the device as they are held, compressed (`PointCompressed(x, y_is_odd)`): the square root of `PublicKey::decompress` runs there
    /// too.  A key the reference's `decompress` would panic on gives `false`.
    pub fn jubjub_verify_batch(&self, items: &[(PublicKey, ZkScalar, Signature)]) -> Result<Vec<bool>, GpuError> {
        let n = items.len();
        let (mut x, mut odd, mut msg, mut sig) = (Vec::with_capacity(n), Vec::with_capacity(n), Vec::with_capacity(n), Vec::with_capacity(3 * n));
        for (k, m, s) in items {
            x.push(k.0 .0);
            odd.push(k.0 .1 as u8);
            msg.push(*m);
            sig.extend_from_slice(&[s.r.0, s.r.1, s.s]);
        }
        let mut ok = vec![0u8; n];
        check(self.0, unsafe {
            sys::bzk_jubjub_verify_batch_compressed(self.0, scalars_ptr(&x), odd.as_ptr(), scalars_ptr(&msg), scalars_ptr(&sig), n as u64, ok.as_mut_ptr())
        })?;
        Ok(ok.into_iter().map(|b| b != 0).collect())
    }

    /// Bulk `MpnTransaction::verify_signature` (src/zk/mod.rs:610-627), what mempool admission asks per transaction
    /// (src/blockchain/mempool.rs:258): the transactions travel as bincode, like the state entries; keys are decompressed, messages hashed and
    /// signatures checked on the device.
    pub fn mpn_tx_verify_batch(&self, txs: &[MpnTransaction]) -> Result<Vec<bool>, GpuError> {
        let mut bytes = Vec::with_capacity(254 * txs.len());
        for tx in txs {
            bytes.extend_from_slice(&bincode::serialize(tx)?);
        }
        let mut ok = vec![0u8; txs.len()];
        let st = unsafe { sys::bzk_mpn_tx_verify_batch(self.0, bytes.as_ptr(), bytes.len() as u64, txs.len() as u64, ok.as_mut_ptr(), ptr::null_mut()) };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        Ok(ok.into_iter().map(|b| b != 0).collect())
    }

    /// Bulk `JubJub::<PoseidonHasher>::generate_keys(seed)` (src/crypto/jubjub/mod.rs:112-124): both SHA3-256 hashes and `scalar BASE` run on the
    /// device, one lane per seed.  The staged seeds and keys are overwritten in the device workspace before the call returns.
    pub fn jubjub_keys_batch(&self, seeds: &[&[u8]]) -> Result<Vec<(PublicKey, PrivateKey)>, GpuError> {
        let mut off = Vec::with_capacity(seeds.len() + 1);
        let mut data = Vec::new();
        off.push(0u64);
        for m in seeds {
            data.extend_from_slice(m);
            off.push(data.len() as u64);
        }
        let mut out = vec![ZkScalar::default(); 4 * seeds.len()];
        check(self.0, unsafe { sys::bzk_jubjub_keys_batch(self.0, data.as_ptr(), off.as_ptr(), seeds.len() as u64, out.as_mut_ptr() as *mut u8) })?;
        Ok(out
            .chunks_exact(4)
            .map(|k| {
                let point = PointAffine(k[0], k[1]);
                (PublicKey(point.compress()), PrivateKey { public_key: point, randomness: k[2], scalar: k[3] })
            })
            .collect())
    }

    /// Bulk `JubJub::<PoseidonHasher>::sign(sk, msg)` (src/crypto/jubjub/mod.rs:125-150): deterministic, so the signatures are the reference's own.
    /// A throughput signer: the fixed-base walk is fixed-flow but indexes a table by nibbles of the nonce.
    pub fn jubjub_sign_batch(&self, items: &[(PrivateKey, ZkScalar)]) -> Result<Vec<Signature>, GpuError> {
        let n = items.len();
        let (mut keys, mut msg) = (Vec::with_capacity(4 * n), Vec::with_capacity(n));
        for (k, m) in items {
            keys.extend_from_slice(&[k.public_key.0, k.public_key.1, k.randomness, k.scalar]);
            msg.push(*m);
        }
        let mut sig = vec![ZkScalar::default(); 3 * n];
        let mut ok = vec![0u8; n];
        check(self.0, unsafe {
            sys::bzk_jubjub_sign_batch(self.0, scalars_ptr(&keys), scalars_ptr(&msg), n as u64, sig.as_mut_ptr() as *mut u8, ok.as_mut_ptr())
        })?;
        Ok(sig.chunks_exact(3).map(|s| Signature { r: PointAffine(s[0], s[1]), s: s[2] }).collect())
    }

    /// The signing step of `TxBuilder::create_mpn_transaction` for many transactions (`tx.sign(&key)`, src/wallet/tx_builder.rs:304: `sig = JubJub::sign(key, tx.hash())`), with the hash, the
    /// decompression of `dst` and the check that `src_pub_key` belongs to the key on the device.  Returns, per transaction, whether it was signed
    /// (`false`: `dst` does not decompress or `src_pub_key` is not the key's; `sig` is left as it was).
    pub fn mpn_txs_sign(&self, keys: &[PrivateKey], txs: &mut [MpnTransaction]) -> Result<Vec<bool>, GpuError> {
        assert!(keys.len() == txs.len());
        let mut flat = Vec::with_capacity(4 * keys.len());
        for k in keys {
            flat.extend_from_slice(&[k.public_key.0, k.public_key.1, k.randomness, k.scalar]);
        }
        let mut bytes = Vec::with_capacity(254 * txs.len());
        let mut ends = Vec::with_capacity(txs.len());
        for tx in txs.iter() {
            bytes.extend_from_slice(&bincode::serialize(tx)?);
            ends.push(bytes.len());
        }
        let mut out = vec![0u8; bytes.len()];
        let mut ok = vec![0u8; txs.len()];
        let st = unsafe {
            sys::bzk_mpn_txs_sign(self.0, scalars_ptr(&flat), bytes.as_ptr(), bytes.len() as u64, txs.len() as u64, out.as_mut_ptr(), ok.as_mut_ptr(), ptr::null_mut())
        };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        for (i, tx) in txs.iter_mut().enumerate() {
            if ok[i] != 0 {
                tx.sig = bincode::deserialize(&out[ends[i] - 96..ends[i]])?;
            }
        }
        Ok(ok.into_iter().map(|b| b != 0).collect())
    }

    /// What `TxBuilder::withdraw_mpn` (src/wallet/tx_builder.rs:376-425) computes, for many withdrawals: `mpn_sig = JubJub::sign(key,
    /// Poseidon(payment.fingerprint(), nonce))` and `payment.calldata = Poseidon(pk.x, pk.y, nonce, sig.r.x, sig.r.y, sig.s)`, with the fingerprint
    /// (a SHA3-256 of the payment with its calldata blanked), both hashes and the signature on the device.  Whatever `mpn_sig` and `calldata`
    /// hold on entry is ignored.  Returns, per withdrawal, whether it was signed (`false`: `mpn_address` is not the key's; the withdrawal is left
    /// as it was).  A payment longer than 65 536 bytes is refused (`GpuError::Status`).  A throughput signer, as `jubjub_sign_batch`.
    pub fn mpn_withdraws_sign(&self, keys: &[PrivateKey], txs: &mut [MpnWithdraw]) -> Result<Vec<bool>, GpuError> {
        assert!(keys.len() == txs.len());
        let mut flat = Vec::with_capacity(4 * keys.len());
        for k in keys {
            flat.extend_from_slice(&[k.public_key.0, k.public_key.1, k.randomness, k.scalar]);
        }
        let mut bytes = Vec::with_capacity(277 * txs.len());
        let mut ends = Vec::with_capacity(txs.len() + 1);
        ends.push(0usize);
        for tx in txs.iter() {
            bytes.extend_from_slice(&bincode::serialize(tx)?);
            ends.push(bytes.len());
        }
        let mut out = vec![0u8; bytes.len()];
        let mut ok = vec![0u8; txs.len()];
        let st = unsafe {
            sys::bzk_mpn_withdraws_sign(self.0, scalars_ptr(&flat), bytes.as_ptr(), bytes.len() as u64, txs.len() as u64, out.as_mut_ptr(), ok.as_mut_ptr(), ptr::null_mut())
        };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        for (i, tx) in txs.iter_mut().enumerate() {
            if ok[i] != 0 {
                *tx = bincode::deserialize(&out[ends[i]..ends[i + 1]])?;
            }
        }
        Ok(ok.into_iter().map(|b| b != 0).collect())
    }

    /// Bulk `MpnWithdraw::verify_signature` / `verify_calldata` (src/core/transaction.rs:177-189), what mempool admission
    /// (src/blockchain/mempool.rs:246-258) and the withdraw builder (src/mpn/withdraw.rs:77) ask per withdrawal: `(signature ok, calldata ok)`.
    /// The withdrawals travel as bincode; the fingerprint (SHA3-256 of the payment with its calldata blanked), the key decompression, both Poseidon
    /// hashes and the signature check run on the device.  A payment longer than 65 536 bytes is refused (`GpuError::Status`).
    pub fn mpn_withdraw_verify_batch(&self, txs: &[MpnWithdraw]) -> Result<Vec<(bool, bool)>, GpuError> {
        let mut bytes = Vec::with_capacity(277 * txs.len());
        for tx in txs {
            bytes.extend_from_slice(&bincode::serialize(tx)?);
        }
        let mut ok = vec![0u8; txs.len()];
        let st =
            unsafe { sys::bzk_mpn_withdraw_verify_batch(self.0, bytes.as_ptr(), bytes.len() as u64, txs.len() as u64, ok.as_mut_ptr(), ptr::null_mut()) };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        Ok(ok.into_iter().map(|b| (b & 1 != 0, b & 2 != 0)).collect())
    }

    /// Bulk `hash_to_scalar` (src/zk/mod.rs:218-220): `ZkScalar::new(sha3_256(msg))` per message, one device lane each.
    pub fn sha3_256_batch(&self, msgs: &[&[u8]]) -> Result<Vec<ZkScalar>, GpuError> {
        let mut off = Vec::with_capacity(msgs.len() + 1);
        let mut data = Vec::new();
        off.push(0u64);
        for m in msgs {
            data.extend_from_slice(m);
            off.push(data.len() as u64);
        }
        let mut out = vec![ZkScalar::default(); msgs.len()];
        check(self.0, unsafe {
            sys::bzk_sha3_256_batch(self.0, data.as_ptr(), off.as_ptr(), msgs.len() as u64, ptr::null_mut(), out.as_mut_ptr() as *mut u8)
        })?;
        Ok(out)
    }

    /// Bulk `ContractDeposit::verify_signature` (src/core/transaction.rs:192-202), what mempool admission (src/blockchain/mempool.rs:241-258) asks
    /// per deposit, and whether `mpn_address` decompresses (src/blockchain/ops/apply_deposit.rs:8 needs the point): `(signature ok, address ok)`.
    /// The deposits travel as bincode; SHA-512, the reduction mod l, the group equation and the key decompression run on the device.  A payment
    /// without a signature gives `false`; a payment longer than 65 536 bytes is refused (`GpuError::Status`).  A host built against an `ed25519`
    /// release older than 1.3 calls `sys::bzk_mpn_set_wire_flags(sys::BZK_WORK_SIG_LEN_PREFIXED)` once before.
    pub fn mpn_deposit_verify_batch(&self, txs: &[MpnDeposit]) -> Result<Vec<(bool, bool)>, GpuError> {
        let mut bytes = Vec::with_capacity(246 * txs.len());
        for tx in txs {
            bytes.extend_from_slice(&bincode::serialize(tx)?);
        }
        let mut ok = vec![0u8; txs.len()];
        let st =
            unsafe { sys::bzk_mpn_deposit_verify_batch(self.0, bytes.as_ptr(), bytes.len() as u64, txs.len() as u64, ok.as_mut_ptr(), ptr::null_mut()) };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        Ok(ok.into_iter().map(|b| (b & 1 != 0, b & 2 != 0)).collect())
    }

    /// Bulk `tx.verify_signature()` and `tx.hash()` (src/core/transaction.rs:383-397): the fourth arm of
    /// `GeneralTransaction::verify_signature` (src/core/mod.rs:163-170).  The transactions travel as bincode; the device hashes
    /// `bincode(tx.sig_state_excluded())` in place from each record.  `(verified, hash)` per transaction.
    pub fn l1_tx_verify_batch(&self, txs: &[Transaction]) -> Result<Vec<(bool, [u8; 32])>, GpuError> {
        let mut bytes = Vec::new();
        for tx in txs {
            bytes.extend_from_slice(&bincode::serialize(tx)?);
        }
        let (mut ok, mut hash) = (vec![0u8; txs.len()], vec![0u8; 32 * txs.len()]);
        let form = 0u32; // BZK_L1_FORM_TX: the records are bincode(Transaction)
        let st =
            unsafe { sys::bzk_l1_tx_verify_batch(self.0, bytes.as_ptr(), bytes.len() as u64, txs.len() as u64, form, ok.as_mut_ptr(), hash.as_mut_ptr()) };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        Ok(ok.iter().zip(hash.chunks_exact(32)).map(|(b, h)| (*b != 0, h.try_into().unwrap())).collect())
    }

    /// `MerkleTree::<Sha3Hasher>::new(leaves.to_vec()).root()` (src/crypto/merkle.rs:79-108).  One small tree is a chain of dependent launches:
    /// the value is in `block_bodies_check`, which builds many blocks' trees level by level together.
    pub fn sha3_merkle_root(&self, leaves: &[[u8; 32]]) -> Result<[u8; 32], GpuError> {
        let count = [leaves.len() as u64];
        let mut root = [0u8; 32];
        check(self.0, unsafe {
            sys::bzk_sha3_merkle_roots(self.0, leaves.as_ptr() as *const u8, count.as_ptr(), 1, root.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok(root)
    }

    /// The cryptographic part of validating block bodies (src/blockchain/ops/apply_block.rs:47 and :88) for many fetched blocks in one call:
    /// per block, whether every transaction's signature verifies and `block.merkle_tree().root()`, which the caller compares with
    /// `block.header.block_root`.
    pub fn block_bodies_check(&self, blocks: &[Block]) -> Result<Vec<(bool, [u8; 32])>, GpuError> {
        let (mut bytes, mut count) = (Vec::new(), Vec::with_capacity(blocks.len()));
        for b in blocks {
            for tx in &b.body {
                bytes.extend_from_slice(&bincode::serialize(tx)?);
            }
            count.push(b.body.len() as u64);
        }
        let (mut ok, mut roots) = (vec![0u8; blocks.len()], vec![0u8; 32 * blocks.len()]);
        let st = unsafe {
            sys::bzk_block_bodies_check(self.0, bytes.as_ptr(), bytes.len() as u64, count.as_ptr(), blocks.len() as u64, ok.as_mut_ptr(),
                                        roots.as_mut_ptr(), ptr::null_mut(), ptr::null_mut())
        };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        Ok(ok.iter().zip(roots.chunks_exact(32)).map(|(b, r)| (*b != 0, r.try_into().unwrap())).collect())
    }

    /// The per-update checks of `update_contract` (src/blockchain/ops/apply_tx/update_contract/mod.rs:28-116) for the `UpdateContract`
    /// transactions `txs` of ONE contract, in chain order: transaction j's updates are checked at `height0 + j`, the first update against
    /// `state0`, every later one against the `next_state` its predecessor claims.  Per update: the `BZK_UPD_*` bits (PROOF, SIGS, ROUTE; 0x80
    /// alone for a Mint), `aux_data.state_hash` and the commitment.  The first update whose bits are not all set is where the sequence breaks.
    /// Balances, nonces, fees and the delta / state-root check after the updates stay with the caller.
    pub fn check_contract_updates(&self, contract_id: ContractId, contract: &ZkContract, txs: &[&[ContractUpdate]], height0: u64,
                                  state0: ZkScalar) -> Result<Vec<(u8, ZkScalar, ZkScalar)>, GpuError> {
        fn key_bytes(vk: &ZkVerifierKey) -> Result<Vec<u8>, GpuError> {
            #[allow(unreachable_patterns)]
            match vk {
                ZkVerifierKey::Groth16(k) => Ok(bincode::serialize(&**k)?),
                _ => Ok(Vec::new()), // no Groth16 key: refused by the call
            }
        }
        let mut keys: Vec<(Vec<u8>, u8)> = Vec::new();
        for f in &contract.deposit_functions {
            keys.push((key_bytes(&f.verifier_key)?, f.log4_payment_capacity));
        }
        for f in &contract.withdraw_functions {
            keys.push((key_bytes(&f.verifier_key)?, f.log4_payment_capacity));
        }
        for f in &contract.functions {
            keys.push((key_bytes(&f.verifier_key)?, 0));
        }
        let fns: Vec<sys::bzk_contract_fn> =
            keys.iter().map(|(k, c)| sys::bzk_contract_fn { vk: k.as_ptr(), vk_len: k.len() as u64, log4_payment_capacity: *c }).collect();
        let (nd, nw) = (contract.deposit_functions.len(), contract.withdraw_functions.len());
        let id: ZkScalar = contract_id.into();
        let mut desc = sys::bzk_contract_desc {
            contract_id: [0u8; 32],
            deposit_fns: fns.as_ptr(),
            n_deposit_fns: nd as u32,
            withdraw_fns: unsafe { fns.as_ptr().add(nd) },
            n_withdraw_fns: nw as u32,
            fns: unsafe { fns.as_ptr().add(nd + nw) },
            n_fns: contract.functions.len() as u32,
        };
        desc.contract_id.copy_from_slice(unsafe { std::slice::from_raw_parts(scalars_ptr(std::slice::from_ref(&id)), 32) });
        let (mut bytes, mut count) = (Vec::new(), Vec::with_capacity(txs.len()));
        for updates in txs {
            for u in updates.iter() {
                bytes.extend_from_slice(&bincode::serialize(u)?);
            }
            count.push(updates.len() as u64);
        }
        let n: usize = txs.iter().map(|u| u.len()).sum();
        let mut ok = vec![0u8; n];
        let (mut aux, mut commit) = (vec![ZkScalar::default(); n], vec![ZkScalar::default(); n]);
        let st = unsafe {
            sys::bzk_contract_updates_check(self.0, &desc, bytes.as_ptr(), bytes.len() as u64, count.as_ptr(), txs.len() as u64, height0,
                                            scalars_ptr(std::slice::from_ref(&state0)), ok.as_mut_ptr(), aux.as_mut_ptr() as *mut u8,
                                            commit.as_mut_ptr() as *mut u8)
        };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        Ok(ok.into_iter().zip(aux).zip(commit).map(|((o, a), c)| (o, a, c)).collect())
    }

    /// Bulk `Ed25519::verify(pk, msg, sig)` (src/crypto/ed25519.rs:81-83: ed25519-dalek 1 `PublicKey::verify`, the non-strict verifier) over raw
    /// bytes: 32-byte keys, 64-byte signatures.  What src/blockchain/ops/apply_block.rs:88 asks per transaction of a block.
    pub fn ed25519_verify_batch(&self, items: &[(&[u8; 32], &[u8], &[u8; 64])]) -> Result<Vec<bool>, GpuError> {
        let n = items.len();
        let (mut pk, mut sig, mut data, mut off) = (Vec::with_capacity(32 * n), Vec::with_capacity(64 * n), Vec::new(), Vec::with_capacity(n + 1));
        off.push(0u64);
        for (k, m, s) in items {
            pk.extend_from_slice(&k[..]);
            sig.extend_from_slice(&s[..]);
            data.extend_from_slice(m);
            off.push(data.len() as u64);
        }
        let mut ok = vec![0u8; n];
        check(self.0, unsafe {
            sys::bzk_ed25519_verify_batch(self.0, pk.as_ptr(), data.as_ptr(), off.as_ptr(), sig.as_ptr(), n as u64, ok.as_mut_ptr())
        })?;
        Ok(ok.into_iter().map(|b| b != 0).collect())
    }

    /// Bulk `Ed25519::<Sha3_256>::generate_keys(seed)` (src/crypto/ed25519.rs:70-77): SHA3-256, SHA-512 and `[a]B` run on the device, one lane per
    /// seed.  Every key is the 64 bytes of `Keypair::to_bytes()` (secret | public).  The staged seeds and keys are overwritten in the device
    /// workspace before the call returns.
    pub fn ed25519_keys_batch(&self, seeds: &[&[u8]]) -> Result<Vec<[u8; 64]>, GpuError> {
        let mut off = Vec::with_capacity(seeds.len() + 1);
        let mut data = Vec::new();
        off.push(0u64);
        for m in seeds {
            data.extend_from_slice(m);
            off.push(data.len() as u64);
        }
        let mut out = vec![[0u8; 64]; seeds.len()];
        check(self.0, unsafe { sys::bzk_ed25519_keys_batch(self.0, data.as_ptr(), off.as_ptr(), seeds.len() as u64, out.as_mut_ptr() as *mut u8) })?;
        Ok(out)
    }

    /// Bulk `Ed25519::sign(sk, msg)` (src/crypto/ed25519.rs:78-80: ed25519-dalek 1 `Keypair::sign`, RFC 8032 5.1.6) over raw bytes: 64-byte
    /// keypairs in, 64-byte signatures out.  Deterministic, so the signatures are dalek's own.  A throughput signer: the fixed-base walk is
    /// fixed-flow but indexes a table by nibbles of the nonce.
    pub fn ed25519_sign_batch(&self, items: &[(&[u8; 64], &[u8])]) -> Result<Vec<[u8; 64]>, GpuError> {
        let n = items.len();
        let (mut keys, mut data, mut off) = (Vec::with_capacity(64 * n), Vec::new(), Vec::with_capacity(n + 1));
        off.push(0u64);
        for (k, m) in items {
            keys.extend_from_slice(&k[..]);
            data.extend_from_slice(m);
            off.push(data.len() as u64);
        }
        let mut out = vec![[0u8; 64]; n];
        check(self.0, unsafe {
            sys::bzk_ed25519_sign_batch(self.0, keys.as_ptr(), data.as_ptr(), off.as_ptr(), n as u64, out.as_mut_ptr() as *mut u8)
        })?;
        Ok(out)
    }

    /// `TxBuilder::sign_deposit` (src/wallet/tx_builder.rs:63-66) for many deposits: `payment.sig = Some(sign(bincode(payment with sig None)))`,
    /// hashed in place on the device.  `keys[i]` is the 64-byte keypair of deposit i.  Returns, per deposit, whether it was signed (`false`:
    /// `payment.src` is not the key's public half; `sig` is left as it was).
    pub fn mpn_deposits_sign(&self, keys: &[[u8; 64]], txs: &mut [MpnDeposit]) -> Result<Vec<bool>, GpuError> {
        assert!(keys.len() == txs.len());
        let mut bytes = Vec::with_capacity(246 * txs.len());
        for tx in txs.iter() {
            bytes.extend_from_slice(&bincode::serialize(tx)?);
        }
        let n = txs.len();
        let (mut sig, mut ok, mut out_len) = (vec![0u8; 64 * n], vec![0u8; n], 0u64);
        let st = unsafe {
            sys::bzk_mpn_deposits_sign(self.0, keys.as_ptr() as *const u8, bytes.as_ptr(), bytes.len() as u64, n as u64, sig.as_mut_ptr(),
                                       ok.as_mut_ptr(), ptr::null_mut(), 0, &mut out_len)
        };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        for (i, tx) in txs.iter_mut().enumerate() {
            if ok[i] != 0 {
                tx.payment.sig = Some(bincode::deserialize(&sig[64 * i..64 * i + 64])?);
            }
        }
        Ok(ok.into_iter().map(|b| b != 0).collect())
    }

    /// `TxBuilder::sign_tx` (src/wallet/tx_builder.rs:67-70) for many transactions of any `TransactionData` variant:
    /// `tx.sig = Signature::Signed(sign(bincode(tx.sig_state_excluded())))`, hashed in place on the device.  Returns, per transaction, whether it
    /// was signed (`false`: `src` is `None` or not the key's public half; `sig` is left as it was) and `tx.hash()`.
    pub fn l1_txs_sign(&self, keys: &[[u8; 64]], txs: &mut [Transaction]) -> Result<Vec<(bool, [u8; 32])>, GpuError> {
        assert!(keys.len() == txs.len());
        let mut bytes = Vec::new();
        for tx in txs.iter() {
            bytes.extend_from_slice(&bincode::serialize(tx)?);
        }
        let n = txs.len();
        let (mut sig, mut ok, mut hash, mut out_len) = (vec![0u8; 64 * n], vec![0u8; n], vec![0u8; 32 * n], 0u64);
        let form = 0u32; // BZK_L1_FORM_TX: the records are bincode(Transaction)
        let st = unsafe {
            sys::bzk_l1_txs_sign(self.0, keys.as_ptr() as *const u8, bytes.as_ptr(), bytes.len() as u64, n as u64, form, sig.as_mut_ptr(),
                                 ok.as_mut_ptr(), hash.as_mut_ptr(), ptr::null_mut(), 0, &mut out_len)
        };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(self.0, st)?;
        for (i, tx) in txs.iter_mut().enumerate() {
            if ok[i] != 0 {
                tx.sig = bazuka::core::Signature::Signed(bincode::deserialize(&sig[64 * i..64 * i + 64])?);
            }
        }
        Ok(ok.iter().zip(hash.chunks_exact(32)).map(|(b, h)| (*b != 0, h.try_into().unwrap())).collect())
    }

    /// Bulk `groth16_verify` (src/zk/groth16/mod.rs:67-121) for proofs of ONE verifying key, one device lane per proof: what
    /// src/blockchain/ops/apply_tx/update_contract/mod.rs:100 asks per `ContractUpdate` and `MpnWork::verify` (src/mpn/mod.rs:281-295) per posted
    /// solution.  `vk` = bincode(Groth16VerifyingKey), every item = (its public inputs as 32-byte Montgomery scalars, the 387-byte proof); all
    /// items carry the same number of inputs.
    pub fn groth16_verify_batch(&self, vk: &[u8], items: &[(&[[u8; 32]], &[u8; 387])]) -> Result<Vec<bool>, GpuError> {
        let n = items.len();
        let n_inputs = items.first().map_or(0, |(x, _)| x.len());
        let (mut inputs, mut proofs) = (Vec::with_capacity(32 * n_inputs * n), Vec::with_capacity(387 * n));
        for (x, p) in items {
            if x.len() != n_inputs {
                return Err(GpuError::Status(sys::BZK_E_ARG, "groth16_verify_batch: every proof of a call has the same number of inputs".into()));
            }
            for s in x.iter() {
                inputs.extend_from_slice(&s[..]);
            }
            proofs.extend_from_slice(&p[..]);
        }
        let mut ok = vec![0u8; n];
        check(self.0, unsafe {
            sys::bzk_groth16_verify_batch(self.0, vk.as_ptr(), vk.len() as u64, inputs.as_ptr(), n_inputs as u32, proofs.as_ptr(), n as u64, ok.as_mut_ptr())
        })?;
        Ok(ok.into_iter().map(|b| b != 0).collect())
    }

    /// The same for proofs of SEVERAL keys in one call - a block's Deposit, Withdraw and Update proofs, or the mix `MpnWork::verify` meets: the
    /// device runs one set of launches for all keys instead of one per key.  `keys` = bincode(Groth16VerifyingKey) each; every item = (the index
    /// of its key, its public inputs, the proof), in any order; an item's number of inputs is its key's.  Verdicts come back in item order.
    pub fn groth16_verify_batch_keys(&self, keys: &[&[u8]], items: &[(usize, &[[u8; 32]], &[u8; 387])]) -> Result<Vec<bool>, GpuError> {
        let n = items.len();
        let mut n_inputs: Vec<Option<u32>> = vec![None; keys.len()];
        let (mut vks, mut vk_off) = (Vec::new(), vec![0u64]);
        for k in keys {
            vks.extend_from_slice(k);
            vk_off.push(vks.len() as u64);
        }
        let (mut key_of, mut inputs, mut proofs) = (Vec::with_capacity(n), Vec::new(), Vec::with_capacity(387 * n));
        for (k, x, p) in items {
            if *k >= keys.len() || *n_inputs[*k].get_or_insert(x.len() as u32) != x.len() as u32 {
                return Err(GpuError::Status(sys::BZK_E_ARG, "groth16_verify_batch_keys: a key index out of range, or two proofs of one key with different numbers of inputs".into()));
            }
            key_of.push(*k as u32);
            for s in x.iter() {
                inputs.extend_from_slice(&s[..]);
            }
            proofs.extend_from_slice(&p[..]);
        }
        let n_inputs: Vec<u32> = n_inputs.into_iter().map(|c| c.unwrap_or(0)).collect();
        let mut ok = vec![0u8; n];
        check(self.0, unsafe {
            sys::bzk_groth16_verify_batch_keys(self.0, keys.len() as u32, vks.as_ptr(), vk_off.as_ptr(), n_inputs.as_ptr(), key_of.as_ptr(), inputs.as_ptr(), proofs.as_ptr(), n as u64, ok.as_mut_ptr())
        })?;
        Ok(ok.into_iter().map(|b| b != 0).collect())
    }

    /// The order-r test of `G1Affine::from_uncompressed` (bls12_381 `is_torsion_free`) for raw points (x | y, little-endian Montgomery limbs),
    /// one device lane per point: 1 = in the subgroup, 0 = on the curve outside it, 2 = not a finite curve point.
    pub fn subgroup_check_g1(&self, pts: &[[u8; 96]]) -> Result<Vec<u8>, GpuError> {
        let mut ok = vec![0u8; pts.len()];
        check(self.0, unsafe {
            sys::bzk_g1_subgroup_check_batch(self.0, pts.as_ptr() as *const u8, ptr::null(), pts.len() as u64, ok.as_mut_ptr())
        })?;
        Ok(ok)
    }

    /// The same for G2 (x.c0 | x.c1 | y.c0 | y.c1).
    pub fn subgroup_check_g2(&self, pts: &[[u8; 192]]) -> Result<Vec<u8>, GpuError> {
        let mut ok = vec![0u8; pts.len()];
        check(self.0, unsafe {
            sys::bzk_g2_subgroup_check_batch(self.0, pts.as_ptr() as *const u8, ptr::null(), pts.len() as u64, ok.as_mut_ptr())
        })?;
        Ok(ok)
    }

    /// `k * P` for many raw G1 points of the order-r subgroup and ONE scalar (32-byte Montgomery limbs), one device lane per point: the points
    /// in canonical affine, and per point whether the product is the identity (its record is 96 zero bytes then).
    pub fn g1_scale_batch(&self, pts: &[[u8; 96]], k: &[u8; 32]) -> Result<(Vec<[u8; 96]>, Vec<bool>), GpuError> {
        let (mut out, mut inf) = (vec![[0u8; 96]; pts.len()], vec![0u8; pts.len()]);
        check(self.0, unsafe {
            sys::bzk_g1_scale_batch(self.0, pts.as_ptr() as *const u8, pts.len() as u64, k.as_ptr(), out.as_mut_ptr() as *mut u8, inf.as_mut_ptr())
        })?;
        Ok((out, inf.into_iter().map(|b| b != 0).collect()))
    }

    /// The phase-2 step of a ceremony on a bellman `Parameters` file: delta times `d` (h and l times 1 / d on the device).  This re-keys delta
    /// alone: it is one contribution, not a ceremony.
    pub fn bellman_params_rekey(&self, params: &[u8], d: &[u8; 32]) -> Result<Vec<u8>, GpuError> {
        let mut size = 0u64;
        check(self.0, unsafe { sys::bzk_bellman_params_rekey(self.0, params.as_ptr(), params.len() as u64, d.as_ptr(), ptr::null_mut(), 0, &mut size) })?;
        let mut out = vec![0u8; size as usize];
        check(self.0, unsafe {
            sys::bzk_bellman_params_rekey(self.0, params.as_ptr(), params.len() as u64, d.as_ptr(), out.as_mut_ptr(), size, ptr::null_mut())
        })?;
        Ok(out)
    }

    /// Is `after` a re-key of `before` by some scalar?  `Ok(None)`: yes; `Ok(Some((array, index, code)))`: the first failure (arrays as
    /// bzk_bellman_params_check names them).  The verdict is only as good as the secrecy of `seed` from whoever made `after`.
    pub fn bellman_params_rekey_check(&self, before: &[u8], after: &[u8], seed: &[u8; 32]) -> Result<Option<(u64, u64, u64)>, GpuError> {
        let mut report = [0u64; 4];
        let st = unsafe {
            sys::bzk_bellman_params_rekey_check(self.0, before.as_ptr(), before.len() as u64, after.as_ptr(), after.len() as u64, seed.as_ptr(), report.as_mut_ptr())
        };
        if st < 0 {
            check(self.0, st)?;
        }
        Ok(if st == 1 { None } else { Some((report[0], report[1], report[2])) })
    }

    /// `k_i * P_i` for raw G1 points of the order-r subgroup and one scalar PER point (32-byte Montgomery limbs), one device lane per point:
    /// the points in canonical affine, and per point whether the product is the identity (its record is zero bytes then).
    pub fn g1_mul_batch(&self, pts: &[[u8; 96]], scalars: &[[u8; 32]]) -> Result<(Vec<[u8; 96]>, Vec<bool>), GpuError> {
        assert_eq!(pts.len(), scalars.len());
        let (mut out, mut inf) = (vec![[0u8; 96]; pts.len()], vec![0u8; pts.len()]);
        check(self.0, unsafe {
            sys::bzk_g1_mul_batch(self.0, pts.as_ptr() as *const u8, scalars.as_ptr() as *const u8, pts.len() as u64, 0, out.as_mut_ptr() as *mut u8, inf.as_mut_ptr())
        })?;
        Ok((out, inf.into_iter().map(|b| b != 0).collect()))
    }

    /// The same on G2 (x.c0 | x.c1 | y.c0 | y.c1).
    pub fn g2_mul_batch(&self, pts: &[[u8; 192]], scalars: &[[u8; 32]]) -> Result<(Vec<[u8; 192]>, Vec<bool>), GpuError> {
        assert_eq!(pts.len(), scalars.len());
        let (mut out, mut inf) = (vec![[0u8; 192]; pts.len()], vec![0u8; pts.len()]);
        check(self.0, unsafe {
            sys::bzk_g2_mul_batch(self.0, pts.as_ptr() as *const u8, scalars.as_ptr() as *const u8, pts.len() as u64, 0, out.as_mut_ptr() as *mut u8, inf.as_mut_ptr())
        })?;
        Ok((out, inf.into_iter().map(|b| b != 0).collect()))
    }

    /// `c * s^(start + i) * P_i`, the scalars made on the device; `c` and `s` are treated as secrets by the library (its copies are overwritten).
    pub fn g1_mul_powers(&self, pts: &[[u8; 96]], c: &[u8; 32], s: &[u8; 32], start: u64) -> Result<(Vec<[u8; 96]>, Vec<bool>), GpuError> {
        let (mut out, mut inf) = (vec![[0u8; 96]; pts.len()], vec![0u8; pts.len()]);
        check(self.0, unsafe {
            sys::bzk_g1_mul_powers(self.0, pts.as_ptr() as *const u8, pts.len() as u64, c.as_ptr(), s.as_ptr(), start, out.as_mut_ptr() as *mut u8, inf.as_mut_ptr())
        })?;
        Ok((out, inf.into_iter().map(|b| b != 0).collect()))
    }

    /// The same on G2.
    pub fn g2_mul_powers(&self, pts: &[[u8; 192]], c: &[u8; 32], s: &[u8; 32], start: u64) -> Result<(Vec<[u8; 192]>, Vec<bool>), GpuError> {
        let (mut out, mut inf) = (vec![[0u8; 192]; pts.len()], vec![0u8; pts.len()]);
        check(self.0, unsafe {
            sys::bzk_g2_mul_powers(self.0, pts.as_ptr() as *const u8, pts.len() as u64, c.as_ptr(), s.as_ptr(), start, out.as_mut_ptr() as *mut u8, inf.as_mut_ptr())
        })?;
        Ok((out, inf.into_iter().map(|b| b != 0).collect()))
    }

    /// One contribution to a powers-of-tau accumulator (the flat blob of include/bzk.h): tau, alpha, beta multiplied by `secrets` =
    /// tau | alpha | beta (Montgomery, none zero).  Returns the new accumulator and the contribution's key tau G2 | alpha G2 | beta G2.
    /// The arithmetic of a contribution, not a ceremony client: no proof of knowledge, no transcript.
    pub fn ptau_contribute(&self, acc: &[u8], secrets: &[u8; 96]) -> Result<(Vec<u8>, [u8; 576]), GpuError> {
        let (mut out, mut key) = (vec![0u8; acc.len()], [0u8; 576]);
        check(self.0, unsafe {
            sys::bzk_ptau_contribute(self.0, acc.as_ptr(), acc.len() as u64, secrets.as_ptr(), out.as_mut_ptr(), out.len() as u64, key.as_mut_ptr())
        })?;
        Ok((out, key))
    }

    /// Is `after` a well-formed accumulator and, with `step` = (before, key), one contribution on top of `before`?  `Ok(None)`: yes;
    /// `Ok(Some((array, index, code)))`: the first failure (0 header or lengths, 1 tau_g1, 2 tau_g2, 3 alpha_g1, 4 beta_g1, 5 beta_g2, 6 key).
    /// The verdict is only as good as the secrecy of `seed` from whoever made `after`.
    pub fn ptau_check(&self, step: Option<(&[u8], &[u8; 576])>, after: &[u8], seed: &[u8; 32]) -> Result<Option<(u64, u64, u64)>, GpuError> {
        let mut report = [0u64; 4];
        let (before, before_len, key) = match step {
            Some((b, k)) => (b.as_ptr(), b.len() as u64, k.as_ptr()),
            None => (ptr::null(), 0, ptr::null()),
        };
        let st = unsafe { sys::bzk_ptau_check(self.0, before, before_len, key, after.as_ptr(), after.len() as u64, seed.as_ptr(), report.as_mut_ptr()) };
        if st < 0 {
            check(self.0, st)?;
        }
        Ok(if st == 1 { None } else { Some((report[0], report[1], report[2])) })
    }

    /// SHA-512 per message, one device lane each
    pub fn sha512_batch(&self, msgs: &[&[u8]]) -> Result<Vec<[u8; 64]>, GpuError> {
        let mut off = Vec::with_capacity(msgs.len() + 1);
        let mut data = Vec::new();
        off.push(0u64);
        for m in msgs {
            data.extend_from_slice(m);
            off.push(data.len() as u64);
        }
        let mut out = vec![[0u8; 64]; msgs.len()];
        check(self.0, unsafe { sys::bzk_sha512_batch(self.0, data.as_ptr(), off.as_ptr(), msgs.len() as u64, out.as_mut_ptr() as *mut u8) })?;
        Ok(out)
    }

    /// Root of a dense `ZkStateModel::List { log4_size, item_type: Scalar }` (what `ZkStateBuilder::compress` returns for it)
    pub fn merkle4_root(&self, leaves: &[ZkScalar], log4_size: u8) -> Result<ZkScalar, GpuError> {
        assert_eq!(leaves.len(), 1usize << (2 * log4_size));
        let mut root = ZkScalar::default();
        check(self.0, unsafe {
            sys::bzk_merkle4_root(self.0, scalars_ptr(leaves), log4_size as u32, &mut root as *mut _ as *mut u8, ptr::null_mut())
        })?;
        Ok(root)
    }

    /// `ZkStateModel::compress::<PoseidonHasher>(&data)` (src/zk/mod.rs:392-399) for any model over sparse pairs
    pub fn compress(&self, model: &ZkStateModel, data: &ZkDataPairs) -> Result<ZkCompressedState, DeviceStateError> {
        let m = bincode::serialize(model).map_err(GpuError::from)?;
        let d = bincode::serialize(data).map_err(GpuError::from)?;
        let mut out = [0u8; 40];
        let st = unsafe { sys::bzk_state_compress_bincode(self.0, m.as_ptr(), m.len() as u64, d.as_ptr(), d.len() as u64, out.as_mut_ptr()) };
        match st {
            sys::BZK_OK => Ok(bincode::deserialize(&out).map_err(GpuError::from)?),
            // refused exactly where the reference reports LocatorError / NonScalarLocatorError (or panics); device failures as GpuError
            e => Err(state_error(self.0, e)),
        }
    }
}

impl Drop for Gpu {
    fn drop(&mut self) {
        unsafe { sys::bzk_ctx_destroy(self.0) }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// `KvStoreStateManager<H>` (src/zk/state/mod.rs:29-31) for ONE contract, values resident on the device.  The reference's functions
// are static over a `KvStore` and a `ContractId`; here the handle IS the contract's store.  One `update_contract` is one batched
// plan on the GPU (every touched node hashed once) instead of depth-many hashes and KV reads per pair.
// ---------------------------------------------------------------------------------------------------------------------------
pub struct DeviceStateManager<'g> {
    st: *mut sys::bzk_state,
    gpu: &'g Gpu,
}
unsafe impl Send for DeviceStateManager<'_> {}

/// What a `DeviceStateManager` call can fail with: the reference's own `StateManagerError` where the library REFUSED the request
/// (nothing changed), or a device-side failure the reference has no variant for (out of HBM while the value store grows; a device
/// error in the middle of an update, after which the handle answers `BZK_E_DEVICE` to everything).  Never a panic.
#[derive(thiserror::Error, Debug)]
pub enum DeviceStateError {
    #[error(transparent)]
    State(#[from] StateManagerError),
    #[error(transparent)]
    Gpu(#[from] GpuError),
}

/// Maps a non-OK status of a `bzk_state_*` call.  `BZK_E_ARG` = refused: `bzk_last_refusal` says which of the reference's errors it
/// stands for (src/zk/state/mod.rs:12-27, src/zk/mod.rs:348-351); anything else is a device / allocation failure and travels as
/// `GpuError::Status` with `bzk_last_error`'s text.
fn state_error(ctx: *mut sys::bzk_ctx, st: i32) -> DeviceStateError {
    if st == sys::BZK_E_ARG {
        return DeviceStateError::State(match unsafe { sys::bzk_last_refusal(ctx) } {
            sys::BZK_REFUSE_NON_SCALAR_LOCATOR => StateManagerError::NonScalarLocatorError,
            sys::BZK_REFUSE_NON_TREE_LOCATOR => StateManagerError::NonTreeLocatorError,
            // InvalidLocator proper; a duplicate locator / a non-canonical value cannot be expressed by the Rust types that produced
            // the bincode (a HashMap key occurs once, a ZkScalar is a residue) and malformed bincode cannot come out of `serialize`:
            // all of them mean "this request names something the state does not have"
            _ => StateManagerError::LocatorError(ZkLocatorError::InvalidLocator),
        });
    }
    DeviceStateError::Gpu(check(ctx, st).unwrap_err())
}

impl<'g> DeviceStateManager<'g> {
    /// an empty contract of this model (`ZkCompressedState::empty::<H>(model)`, src/zk/mod.rs:557-562)
    pub fn new(gpu: &'g Gpu, model: &ZkStateModel) -> Result<Self, GpuError> {
        let m = bincode::serialize(model)?;
        let mut st = ptr::null_mut();
        check(gpu.0, unsafe { sys::bzk_state_create(gpu.0, m.as_ptr(), m.len() as u64, &mut st) })?;
        Ok(DeviceStateManager { st, gpu })
    }

    /// `update_contract(db, id, patch, target_height)` (src/zk/state/mod.rs:286-308): all or nothing
    pub fn update_contract(&mut self, patch: &ZkDeltaPairs, target_height: u64) -> Result<ZkCompressedState, DeviceStateError> {
        let d = bincode::serialize(patch).map_err(GpuError::from)?;
        let mut out = [0u8; 40];
        match unsafe { sys::bzk_state_update_bincode(self.st, d.as_ptr(), d.len() as u64, target_height, out.as_mut_ptr()) } {
            sys::BZK_OK => Ok(bincode::deserialize(&out).map_err(GpuError::from)?),
            e => Err(state_error(self.gpu.0, e)),
        }
    }

    /// A chain of deltas in one pass, every root checked (`update_contract/mod.rs:129-144` per block: apply the transaction's `ZkDeltaPairs`, then require
    /// `root == cont_account.compressed_state`): `update_contract(patches[j], target_heights[j])` for j = 0, 1, .. while each is accepted and gives
    /// `claims[j]` (None: nothing can mismatch).  Returns how many deltas are part of the state now, the verdict of each (`sys::BZK_CHAIN_APPLIED`, `sys::BZK_CHAIN_MISMATCH`, `sys::BZK_CHAIN_REFUSED`, `sys::BZK_CHAIN_NOT_REACHED`), and the
    /// state each applied (or mismatching) delta produces.  A refused delta is a verdict, not an error; it and everything behind it leave no trace.
    pub fn update_contract_chain(&mut self, patches: &[ZkDeltaPairs], target_heights: &[u64], claims: Option<&[ZkCompressedState]>)
                                 -> Result<(usize, Vec<u8>, Vec<ZkCompressedState>), DeviceStateError> {
        let m = patches.len();
        assert!(target_heights.len() == m && claims.map_or(true, |c| c.len() == m), "one height and one claim per delta");
        let (mut blobs, mut off) = (Vec::new(), vec![0u64]);
        for p in patches {
            blobs.extend_from_slice(&bincode::serialize(p).map_err(GpuError::from)?);
            off.push(blobs.len() as u64);
        }
        let mut claim_bytes = Vec::new();
        for c in claims.unwrap_or(&[]) {
            claim_bytes.extend_from_slice(&bincode::serialize(c).map_err(GpuError::from)?);
        }
        let (mut states, mut verdict, mut applied) = (vec![0u8; 40 * m], vec![0u8; m], 0u64);
        if blobs.is_empty() {
            blobs.push(0);
        }
        let st = unsafe {
            sys::bzk_state_update_chain_bincode(self.st, m as u64, blobs.as_ptr(), off.as_ptr(), target_heights.as_ptr(),
                                                if claims.is_some() { claim_bytes.as_ptr() } else { ptr::null() }, 0, states.as_mut_ptr(),
                                                verdict.as_mut_ptr(), &mut applied)
        };
        if st != sys::BZK_OK {
            return Err(state_error(self.gpu.0, st));
        }
        let mut out = Vec::with_capacity(m);
        for s in states.chunks_exact(40) {
            out.push(bincode::deserialize(s).map_err(GpuError::from)?);
        }
        Ok((applied as usize, verdict, out))
    }

    /// `root` (:274-284) and `height_of` (:210-216)
    pub fn root(&self) -> Result<(ZkCompressedState, u64), DeviceStateError> {
        let (mut hash, mut size, mut height) = (ZkScalar::default(), 0u64, 0u64);
        match unsafe { sys::bzk_state_root(self.st, &mut hash as *mut _ as *mut u8, &mut size, &mut height) } {
            sys::BZK_OK => Ok((ZkCompressedState::new(hash, size), height)),
            e => Err(state_error(self.gpu.0, e)),  // BZK_E_DEVICE: an earlier update failed on the device
        }
    }

    /// `get_data` (:422-438) for many locators in one device read
    pub fn get_data(&self, locators: &[ZkDataLocator]) -> Result<Vec<ZkScalar>, DeviceStateError> {
        let mut off = vec![0u64];
        let mut flat = Vec::new();
        for l in locators {
            flat.extend_from_slice(&l.0);
            off.push(flat.len() as u64);
        }
        let mut out = vec![ZkScalar::default(); locators.len()];
        match unsafe { sys::bzk_state_get(self.st, off.as_ptr(), flat.as_ptr(), locators.len() as u64, out.as_mut_ptr() as *mut u8) } {
            sys::BZK_OK => Ok(out),
            e => Err(state_error(self.gpu.0, e)),
        }
    }

    /// `prove(db, id, tree_loc, index)` (:218-264): `Vec<[ZkScalar; 3]>`, leaf level first
    pub fn prove(&self, tree_loc: &ZkDataLocator, index: u64) -> Result<Vec<[ZkScalar; 3]>, DeviceStateError> {
        let mut log4 = 0u32;
        let st = unsafe { sys::bzk_state_prove(self.st, tree_loc.0.as_ptr(), tree_loc.0.len() as u64, ptr::null(), 0, ptr::null_mut(), &mut log4) };
        if st != sys::BZK_OK {
            return Err(state_error(self.gpu.0, st));  // InvalidLocator vs NonTreeLocatorError: told apart by bzk_last_refusal
        }
        let mut out = vec![[ZkScalar::default(); 3]; log4 as usize];
        match unsafe {
            sys::bzk_state_prove(self.st, tree_loc.0.as_ptr(), tree_loc.0.len() as u64, &index, 1, out.as_mut_ptr() as *mut u8, &mut log4)
        } {
            sys::BZK_OK => Ok(out),
            e => Err(state_error(self.gpu.0, e)),  // an index beyond the list: InvalidLocator
        }
    }

    pub fn gpu(&self) -> &Gpu {
        self.gpu
    }
}

impl Drop for DeviceStateManager<'_> {
    fn drop(&mut self) {
        unsafe { sys::bzk_state_free(self.st) }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// `impl ZkHasher` (src/zk/mod.rs:152-155): a static fn, so the context is a process-wide one on device BZK_DEVICE (default 0).
// `hash` of ONE input vector runs on the host (a single Poseidon is a ~50 us job; a PCIe round trip would cost more) through the
// library's own host Poseidon - same parameters, same bytes; the GPU is for `hash_batch`.
// ---------------------------------------------------------------------------------------------------------------------------
static GPU: OnceLock<Mutex<Gpu>> = OnceLock::new();

pub fn shared_gpu() -> &'static Mutex<Gpu> {
    GPU.get_or_init(|| {
        let dev = std::env::var("BZK_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
        Mutex::new(Gpu::new(dev).expect("bazuka-gpu: no usable gfx950 device (libbzk has no CPU fallback)"))
    })
}

#[derive(Debug, Clone, PartialEq, Eq, std::hash::Hash, Default)]
pub struct GpuPoseidonHasher;

impl ZkHasher for GpuPoseidonHasher {
    const MAX_ARITY: usize = 16; // poseidon::MAX_ARITY (src/zk/poseidon/params/mod.rs:25)
    fn hash(vals: &[ZkScalar]) -> ZkScalar {
        let mut out = ZkScalar::default();
        let st = unsafe { sys::bzk_host_poseidon(scalars_ptr(vals), vals.len() as u32, &mut out as *mut _ as *mut u8) };
        assert_eq!(st, sys::BZK_OK, "arity outside 1..=16 (the reference unwraps a missing parameter set here)");
        out
    }
}

impl GpuPoseidonHasher {
    /// the bulk path: n independent hashes of the same arity in one device launch
    pub fn hash_batch(vals: &[ZkScalar], arity: usize) -> Vec<ZkScalar> {
        shared_gpu().lock().unwrap().hash_batch(vals, arity).expect("bzk_poseidon_batch")
    }
}

/// `ZkStateModel::compress` through the shared context (drop-in for `model.compress::<PoseidonHasher>(&data)`)
pub fn compress(model: &ZkStateModel, data: &ZkDataPairs) -> Result<ZkCompressedState, DeviceStateError> {
    shared_gpu().lock().unwrap().compress(model, data)
}

/// The trivial powers-of-tau accumulator for m = 2^log_m (every entry its group's generator); `None` for a log_m outside 1 .. 24.  No device.
pub fn ptau_init(log_m: u32) -> Option<Vec<u8>> {
    let size = unsafe { sys::bzk_ptau_size(log_m) };
    if size == 0 {
        return None;
    }
    let mut out = vec![0u8; size as usize];
    (unsafe { sys::bzk_ptau_init(log_m, out.as_mut_ptr(), size) } == sys::BZK_OK).then(|| out)
}

// ---------------------------------------------------------------------------------------------------------------------------
// Groth16: proving parameters live on the device; `groth16_prove` sits beside `groth16_verify` (src/zk/groth16/mod.rs:67-75).
// ---------------------------------------------------------------------------------------------------------------------------
/// A CRS uploaded once (bellman `Parameters`): from a bellman parameter file + the circuit shape's density maps.
pub struct ProvingParams {
    gpu: Gpu,
    params: *mut sys::bzk_params,
    /// bincode(`Groth16VerifyingKey`) as the library derived it from the file
    pub vk_bincode: Vec<u8>,
}
unsafe impl Send for ProvingParams {}

impl ProvingParams {
    /// `bytes` = `bellman::groth16::Parameters::<Bls12>::write` output; densities = views 4 / 5 of the empty circuit
    pub fn from_bellman(device: i32, bytes: &[u8], n_in: u32, n_aux: u32, a_density: &[u8], b_density: &[u8]) -> Result<Self, GpuError> {
        let gpu = Gpu::new(device)?;
        let mut params = ptr::null_mut();
        let mut vk = vec![0u8; 878 + 97 * n_in as usize];
        check(gpu.0, unsafe {
            sys::bzk_params_load_bellman(gpu.0, bytes.as_ptr(), bytes.len() as u64, n_in, n_aux, a_density.as_ptr(), b_density.as_ptr(),
                                         &mut params, vk.as_mut_ptr(), vk.len() as u64)
        })?;
        Ok(ProvingParams { gpu, params, vk_bincode: vk })
    }

    /// `bellman::groth16::Parameters::<Bls12>::read(reader, checked)` shaped: the whole reader is consumed, `checked = true` also tests every
    /// point for the order-r subgroup (the queries on the device, in the arrays the load uploads).  A failing point is
    /// `GpuError::Status(BZK_E_ARG, ..)` whose text names the array and index; no parameters are left on the device.
    pub fn read<R: std::io::Read>(device: i32, mut reader: R, checked: bool, n_in: u32, n_aux: u32, a_density: &[u8], b_density: &[u8]) -> Result<Self, GpuError> {
        let mut bytes = Vec::new();
        reader.read_to_end(&mut bytes).map_err(|e| GpuError::Status(sys::BZK_E_ARG, format!("Parameters::read: {e}")))?;
        if !checked {
            return Self::from_bellman(device, &bytes, n_in, n_aux, a_density, b_density);
        }
        let gpu = Gpu::new(device)?;
        let mut params = ptr::null_mut();
        let mut vk = vec![0u8; 878 + 97 * n_in as usize];
        let mut report = [0u64; 4];
        check(gpu.0, unsafe {
            sys::bzk_params_load_bellman_checked(gpu.0, bytes.as_ptr(), bytes.len() as u64, n_in, n_aux, a_density.as_ptr(), b_density.as_ptr(),
                                                 &mut params, vk.as_mut_ptr(), vk.len() as u64, report.as_mut_ptr())
        })?;
        Ok(ProvingParams { gpu, params, vk_bincode: vk })
    }

    /// The phase-2 step of a ceremony on these resident parameters: NEW parameters whose delta is `d` times this one's (h and l times 1 / d
    /// on the device, a / b_g1 / b_g2 copied there).  `self` is left as it was; `device` is the device both live on (the new parameters own a
    /// context of their own, as every `ProvingParams` does).  This re-keys delta alone: it is one contribution, not a ceremony.
    pub fn rekey(&self, device: i32, d: &[u8; 32]) -> Result<Self, GpuError> {
        let gpu = Gpu::new(device)?;
        let mut params = ptr::null_mut();
        let mut vk = self.vk_bincode.clone();
        check(gpu.0, unsafe { sys::bzk_params_rekey(gpu.0, self.params, d.as_ptr(), &mut params, vk.as_mut_ptr()) })?;
        Ok(ProvingParams { gpu, params, vk_bincode: vk })
    }

    /// `Parameters::read(.., checked = true)` as a verdict without loading anything: `Ok(None)` when every point passes, else
    /// `Ok(Some([array, index, verdict code, 0]))` of the first failure in file order (array 0 = verifying key head, 1 ic, 2 h, 3 l, 4 a, 5 b_g1, 6 b_g2).
    pub fn check_bellman(gpu: &Gpu, bytes: &[u8]) -> Result<Option<[u64; 4]>, GpuError> {
        let mut report = [0u64; 4];
        let st = unsafe { sys::bzk_bellman_params_check(gpu.0, bytes.as_ptr(), bytes.len() as u64, report.as_mut_ptr()) };
        if st < 0 {
            check(gpu.0, st)?;
        }
        Ok(if st == 1 { None } else { Some(report) })
    }
}

impl Drop for ProvingParams {
    fn drop(&mut self) {
        unsafe { sys::bzk_params_free(self.gpu.0, self.params) }
    }
}

/// A synthesized circuit instance (assignment z and the evaluations A.z, B.z, C.z in pinned host memory)
pub struct Witness(*mut sys::bzk_r1cs);
unsafe impl Send for Witness {}

impl Witness {
    fn view(&self, which: i32) -> (*const u8, u64) {
        let mut bytes = 0u64;
        let p = unsafe { sys::bzk_r1cs_data(self.0, which, &mut bytes) } as *const u8;
        (p, bytes)
    }
    fn assignment(&self) -> sys::bzk_assignment {
        let (z, zb) = self.view(0);
        let (az, ab) = self.view(1);
        let (bz, _) = self.view(2);
        let (cz, _) = self.view(3);
        sys::bzk_assignment { z, az, bz, cz, n_rows: ab / 32, n_vars: zb / 32 }
    }
    /// the five public inputs [commitment, height, state, aux_data, next_state] follow z[0] = 1
    pub fn satisfied(&self) -> bool {
        let mut info = [0u64; 9];
        unsafe { sys::bzk_r1cs_info(self.0, info.as_mut_ptr()) == sys::BZK_OK && info[6] == 0 }
    }
}

impl Drop for Witness {
    fn drop(&mut self) {
        unsafe { sys::bzk_r1cs_free(self.0) }
    }
}

/// The circuit instance of an `MpnWork` for `prover` (commitment = `ZkScalar::new(sha3(bincode((prover, reward))))`,
/// src/mpn/mod.rs:283-285; transitions padded with `::null` ones as `prepare_works` leaves them)
pub fn synthesize_work(work: &MpnWork, prover: &Address) -> Result<Witness, GpuError> {
    let bytes = bincode::serialize(work)?;
    let prover_pub = bincode::serialize(prover)?; // Address = 32-byte ed25519 public key
    let mut w = ptr::null_mut();
    let mut consumed = 0u64;
    check(ptr::null_mut(), unsafe { sys::bzk_mpn_work_decode(bytes.as_ptr(), bytes.len() as u64, 0, &mut w, &mut consumed) })?;
    let mut r1cs = ptr::null_mut();
    let st = unsafe { sys::bzk_mpn_work_synthesize(w, prover_pub.as_ptr(), ptr::null(), 0, 0, &mut r1cs) };
    unsafe { sys::bzk_mpn_work_free(w) };
    check(ptr::null_mut(), st)?;
    Ok(Witness(r1cs))
}

/// Beside `groth16_verify(vk, commitment, prev_height, prev_state, aux_data, next_state, proof) -> bool`
/// (src/zk/groth16/mod.rs:67-75): the prover of the same statement.  The public inputs are those the witness was synthesized
/// with (z[1..=5]); `r`, `s` are the blinding factors bellman's `create_random_proof` draws from its rng.
pub fn groth16_prove(params: &ProvingParams, witness: &Witness, r: ZkScalar, s: ZkScalar) -> Result<Groth16Proof, GpuError> {
    let asg = witness.assignment();
    let mut buf = [0u8; 387];
    check(params.gpu.0, unsafe {
        sys::bzk_groth16_prove(params.gpu.0, params.params, &asg, &r as *const _ as *const u8, &s as *const _ as *const u8, buf.as_mut_ptr())
    })?;
    Ok(bincode::deserialize(&buf)?) // private fields: through bincode, never a pointer cast
}

/// The three matrices of a circuit shape resident on the parameters' device (`bzk_r1cs_mats_load`): what `prove_witness` evaluates A.z, B.z, C.z
/// from.  For a circuit of the caller's own - the reference lets every contract bring its Groth16 key - whose witness comes without evaluations.
/// Read-only after loading; freed on drop (after the last proof from it has returned).
pub struct CircuitMatrices {
    h: *mut sys::bzk_r1cs_mats,
    ctx: *mut sys::bzk_ctx,
}
unsafe impl Send for CircuitMatrices {}
unsafe impl Sync for CircuitMatrices {}

/// One CSR matrix as `bzk_groth16_setup` takes it: `row_ptr` (n_rows + 1), flat variable indices (inputs, then aux), Montgomery coefficients
pub struct CsrMatrix<'a> {
    pub row_ptr: &'a [u32],
    pub col: &'a [u32],
    pub val: &'a [ZkScalar],
}

impl CsrMatrix<'_> {
    fn raw(&self) -> sys::bzk_csr {
        sys::bzk_csr { n_rows: self.row_ptr.len().saturating_sub(1) as u64, row_ptr: self.row_ptr.as_ptr(), col: self.col.as_ptr(), val: scalars_ptr(self.val) }
    }
}

impl CircuitMatrices {
    /// A, B, C over `n_in` inputs (ONE first) and `n_aux` aux variables, rows including bellman's trailing `input_i * 0 = 0` constraints.
    /// A malformed matrix is `GpuError::Status(BZK_E_ARG, ..)` naming the matrix and the row.
    pub fn load(params: &ProvingParams, a: &CsrMatrix<'_>, b: &CsrMatrix<'_>, c: &CsrMatrix<'_>, n_in: u32, n_aux: u32) -> Result<Self, GpuError> {
        assert!(a.col.len() == a.val.len() && b.col.len() == b.val.len() && c.col.len() == c.val.len());
        assert!(!a.row_ptr.is_empty() && !b.row_ptr.is_empty() && !c.row_ptr.is_empty());
        let (ra, rb, rc) = (a.raw(), b.raw(), c.raw());
        let mut h = ptr::null_mut();
        check(params.gpu.0, unsafe { sys::bzk_r1cs_mats_load(params.gpu.0, &ra, &rb, &rc, n_in, n_aux, &mut h) })?;
        Ok(CircuitMatrices { h, ctx: params.gpu.0 })
    }

    /// the same from an instance synthesized with `record_matrices`
    pub fn from_witness(params: &ProvingParams, witness: &Witness) -> Result<Self, GpuError> {
        let mut h = ptr::null_mut();
        check(params.gpu.0, unsafe { sys::bzk_r1cs_mats_from_r1cs(params.gpu.0, witness.0, &mut h) })?;
        Ok(CircuitMatrices { h, ctx: params.gpu.0 })
    }

    /// (rows, variables, nnz(A), nnz(B), nnz(C), distinct coefficients, resident bytes)
    pub fn info(&self) -> [u64; 7] {
        let mut info = [0u64; 8];
        let st = unsafe { sys::bzk_r1cs_mats_info(self.h, info.as_mut_ptr()) };
        assert_eq!(st, sys::BZK_OK);
        [info[0], info[1], info[2], info[3], info[4], info[5], info[6]]
    }
}

impl Drop for CircuitMatrices {
    fn drop(&mut self) {
        unsafe { sys::bzk_r1cs_mats_free(self.ctx, self.h) }
    }
}

/// `groth16_prove` from the assignment `z` alone (inputs with z[0] = 1, then aux): A.z, B.z, C.z are computed on the device from `mats`.
/// `check_satisfied`: one product per constraint first - an unsatisfied witness is `GpuError::Status(BZK_E_UNSAT, ..)` naming the first
/// failing constraint instead of an invalid proof.
pub fn prove_witness(params: &ProvingParams, mats: &CircuitMatrices, z: &[ZkScalar], r: ZkScalar, s: ZkScalar, check_satisfied: bool) -> Result<Groth16Proof, GpuError> {
    let flags: u32 = if check_satisfied { sys::BZK_PROVE_CHECK_SAT } else { 0 };
    let mut buf = [0u8; 387];
    check(params.gpu.0, unsafe {
        sys::bzk_groth16_prove_witness(params.gpu.0, params.params, mats.h, scalars_ptr(z), z.len() as u64, &r as *const _ as *const u8, &s as *const _ as *const u8, flags, buf.as_mut_ptr())
    })?;
    Ok(bincode::deserialize(&buf)?)
}

/// `synthesize_work` with the hash-dependent witness values of the work's transitions LEFT TO THE DEVICE (include/bzk.h: BZK_SYNTH_DEFER): the
/// Poseidon gadget's variables, the Merkle muxes and the root checks - four fifths of a transition - are not evaluated on the host;
/// `groth16_prove_witness` completes them on the GPU before proving.  All three kinds of work (update, deposit, withdraw).
pub fn synthesize_work_deferred(work: &MpnWork, prover: &Address) -> Result<Witness, GpuError> {
    let bytes = bincode::serialize(work)?;
    let prover_pub = bincode::serialize(prover)?;
    let mut w = ptr::null_mut();
    let mut consumed = 0u64;
    check(ptr::null_mut(), unsafe { sys::bzk_mpn_work_decode(bytes.as_ptr(), bytes.len() as u64, 0, &mut w, &mut consumed) })?;
    let mut r1cs = ptr::null_mut();
    let st = unsafe { sys::bzk_mpn_work_synthesize(w, prover_pub.as_ptr(), ptr::null(), 0, sys::BZK_SYNTH_DEFER as i32, &mut r1cs) };
    unsafe { sys::bzk_mpn_work_free(w) };
    check(ptr::null_mut(), st)?;
    Ok(Witness(r1cs))
}

/// `synthesize_work_deferred` with the EdDSA gadget of every Update / Withdraw transition deferred as well (include/bzk.h: BZK_SYNTH_DEFER_SIG): its two
/// 254-step ladders and the signature's tail are computed and filled in on the GPU by `groth16_prove_witness`.  A signature that does not verify arrives as
/// `BZK_E_UNSAT` from the prove call.  Deposit works have no signature gadget: their instance is `synthesize_work_deferred`'s.
pub fn synthesize_work_deferred_sig(work: &MpnWork, prover: &Address) -> Result<Witness, GpuError> {
    let bytes = bincode::serialize(work)?;
    let prover_pub = bincode::serialize(prover)?;
    let mut w = ptr::null_mut();
    let mut consumed = 0u64;
    check(ptr::null_mut(), unsafe { sys::bzk_mpn_work_decode(bytes.as_ptr(), bytes.len() as u64, 0, &mut w, &mut consumed) })?;
    let mut r1cs = ptr::null_mut();
    let st = unsafe { sys::bzk_mpn_work_synthesize(w, prover_pub.as_ptr(), ptr::null(), 0, sys::BZK_SYNTH_DEFER_SIG as i32, &mut r1cs) };
    unsafe { sys::bzk_mpn_work_free(w) };
    check(ptr::null_mut(), st)?;
    Ok(Witness(r1cs))
}

/// `groth16_prove` over the generator's own instance handle: a deferred instance is completed on the device first.  `BZK_E_UNSAT` (a
/// deferred constraint does not hold) arrives as `GpuError::Status`, never as a panic.
pub fn groth16_prove_witness(params: &ProvingParams, witness: &Witness, r: ZkScalar, s: ZkScalar) -> Result<Groth16Proof, GpuError> {
    let mut buf = [0u8; 387];
    check(params.gpu.0, unsafe {
        sys::bzk_groth16_prove_r1cs(params.gpu.0, params.params, witness.0, &r as *const _ as *const u8, &s as *const _ as *const u8, buf.as_mut_ptr())
    })?;
    Ok(bincode::deserialize(&buf)?)
}

/// An instance's assignment resident in HBM (`bzk_r1cs_stage`): the uploads and - for a deferred instance - the device-side fill run on a context of the
/// witness PRODUCER's, so that the prover slot only copies device to device.  The `Witness` it was staged from is kept alive inside (its pinned host arrays are
/// read by the staging stream until `wait` or a prove call has returned); the handle goes back to the staging context's pool on drop.
pub struct Staged<'g> {
    h: *mut sys::bzk_staged,
    _gpu: &'g Gpu,
    _witness: Witness,
}
unsafe impl Send for Staged<'_> {}

impl Gpu {
    /// `bzk_r1cs_stage` on THIS context's stream (a producer's context, not a prover slot's); returns at once
    pub fn stage(&self, witness: Witness) -> Result<Staged<'_>, GpuError> {
        let mut h = ptr::null_mut();
        check(self.0, unsafe { sys::bzk_r1cs_stage(self.0, witness.0, &mut h) })?;
        Ok(Staged { h, _gpu: self, _witness: witness })
    }
}

impl Staged<'_> {
    /// blocks until the staging work has finished; `BZK_E_UNSAT` (a deferred constraint does not hold, or a transition's computed state differs from the
    /// builder's prediction) arrives as `GpuError::Status`, never as a panic
    pub fn wait(&self) -> Result<(), GpuError> {
        check(ptr::null_mut(), unsafe { sys::bzk_staged_wait(self.h) })
    }
    /// one complete array as the device left it (0 z, 1 A.z, 2 B.z, 3 C.z): what `ProvingAssignment` holds after `Circuit::synthesize`
    pub fn read(&self, which: i32) -> Result<Vec<ZkScalar>, GpuError> {
        let mut bytes = 0u64;
        check(ptr::null_mut(), unsafe { sys::bzk_staged_read(self.h, which, ptr::null_mut(), 0, &mut bytes) })?;
        let mut out = vec![ZkScalar::default(); (bytes / 32) as usize];
        check(ptr::null_mut(), unsafe { sys::bzk_staged_read(self.h, which, out.as_mut_ptr() as *mut u8, bytes, ptr::null_mut()) })?;
        Ok(out)
    }
}

impl Drop for Staged<'_> {
    fn drop(&mut self) {
        // the staging stream may still be reading the witness's host arrays: wait before they (and the handle) go
        unsafe {
            let _ = sys::bzk_staged_wait(self.h);
            sys::bzk_staged_free(self.h)
        }
    }
}

/// `groth16_prove` over a staged instance (any context of the same device as the one it was staged on): waits for the staging work in stream order
/// and copies device to device; same proof bytes as `groth16_prove` / `groth16_prove_witness`
pub fn groth16_prove_staged(params: &ProvingParams, staged: &Staged<'_>, r: ZkScalar, s: ZkScalar) -> Result<Groth16Proof, GpuError> {
    let mut buf = [0u8; 387];
    check(params.gpu.0, unsafe {
        sys::bzk_groth16_prove_staged(params.gpu.0, params.params, staged.h, &r as *const _ as *const u8, &s as *const _ as *const u8, buf.as_mut_ptr())
    })?;
    Ok(bincode::deserialize(&buf)?)
}

/// `GET /bincode/mpn/work` -> this -> `POST /bincode/mpn/solution` (src/client/messages.rs:368-388): the `ZkProof` that
/// `work.verify(prover, &proof)` accepts
pub fn prove_work(params: &ProvingParams, work: &MpnWork, prover: &Address, r: ZkScalar, s: ZkScalar) -> Result<ZkProof, GpuError> {
    let w = synthesize_work(work, prover)?;
    Ok(ZkProof::Groth16(Box::new(groth16_prove(params, &w, r, s)?)))
}

// ---------------------------------------------------------------------------------------------------------------------------
// Device groups (include/bzk.h row (e)): one process drives the GPUs of a node.
// ---------------------------------------------------------------------------------------------------------------------------
pub struct DeviceGroup(*mut sys::bzk_mg);
unsafe impl Send for DeviceGroup {}

pub struct GroupBases<'g> {
    group: &'g DeviceGroup,
    h: *mut sys::bzk_mg_bases,
}

impl DeviceGroup {
    /// transport: RCCL all-gather over xGMI when the devices are distinct, host memory otherwise (`BZK_MG_X_AUTO`)
    pub fn new(devices: &[i32]) -> Result<Self, GpuError> {
        let mut h = ptr::null_mut();
        check(ptr::null_mut(), unsafe { sys::bzk_mg_create(devices.as_ptr(), devices.len() as i32, sys::BZK_MG_X_AUTO, &mut h) })?;
        Ok(DeviceGroup(h))
    }
    pub fn world(&self) -> i32 {
        unsafe { sys::bzk_mg_world(self.0) }
    }
    /// what this process could contribute to a process-per-GPU group on `device`: bit 0 = usable gfx950 device, bit 1 = librccl loadable.
    /// A host collects the answers of all ranks BEFORE creating a group on the RCCL transport (`ncclCommInitRank` blocks until every
    /// rank arrives; include/bzk.h)
    pub fn probe(device: i32) -> i32 {
        unsafe { sys::bzk_mg_probe(device) }
    }
    fn fail(&self, st: i32) -> GpuError {
        GpuError::Status(st, unsafe { CStr::from_ptr(sys::bzk_mg_last_error(self.0)).to_string_lossy().into_owned() })
    }
    /// replicate a static G1 base set (raw affine `x | y`, 96 bytes per point) on every device, converted once
    pub fn load_g1_bases(&self, raw: &[u8]) -> Result<GroupBases<'_>, GpuError> {
        let mut h = ptr::null_mut();
        let st = unsafe { sys::bzk_mg_bases_g1_load(self.0, raw.as_ptr(), (raw.len() / 96) as u64, &mut h) };
        if st != sys::BZK_OK {
            return Err(self.fail(st));
        }
        Ok(GroupBases { group: self, h })
    }
    /// one MSM sharded by scalar-window range over the group; returns the packed affine point (97 bytes)
    pub fn msm_g1(&self, bases: &GroupBases<'_>, scalars: &[ZkScalar]) -> Result<[u8; 97], GpuError> {
        let mut out = [0u8; 97];
        let st = unsafe { sys::bzk_mg_msm_g1(self.0, bases.h, scalars_ptr(scalars), scalars.len() as u64, 0, out.as_mut_ptr()) };
        if st != sys::BZK_OK {
            return Err(self.fail(st));
        }
        Ok(out)
    }
}

impl Drop for GroupBases<'_> {
    fn drop(&mut self) {
        unsafe { sys::bzk_mg_bases_free(self.group.0, self.h) }
    }
}

impl Drop for DeviceGroup {
    fn drop(&mut self) {
        unsafe { sys::bzk_mg_destroy(self.0) }
    }
}

/// Host only, parses and nothing else: (transaction index, offset, length) of every `ContractUpdate` of every `UpdateContract` of `contract_id`
/// inside `bytes`, the bincode of `n` consecutive `TransactionAndDelta` (`with_delta`) or `Transaction` records - what `Gpu::block_bodies_check`
/// serializes.  The spans re-slice to the input of `bzk_contract_updates_check`.
pub fn contract_update_spans(bytes: &[u8], n: usize, with_delta: bool, contract_id: ContractId) -> Result<Vec<(u64, u64, u64)>, GpuError> {
    let id: ZkScalar = contract_id.into();
    let form: u32 = if with_delta { 1 } else { 0 }; // BZK_L1_FORM_TX_AND_DELTA / BZK_L1_FORM_TX
    let mut found = 0u64;
    let mut spans: Vec<u64> = Vec::new();
    for _ in 0..2 {
        let st = unsafe {
            sys::bzk_l1_tx_updates(bytes.as_ptr(), bytes.len() as u64, n as u64, form, scalars_ptr(std::slice::from_ref(&id)), spans.as_mut_ptr(),
                                   (spans.len() / 3) as u64, &mut found)
        };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(ptr::null_mut(), st)?;
        if spans.len() as u64 >= 3 * found {
            break;
        }
        spans = vec![0u64; 3 * found as usize];
    }
    Ok(spans.chunks_exact(3).take(found as usize).map(|s| (s[0], s[1], s[2])).collect())
}

/// Its sibling for the state step: per `UpdateContract` of `contract_id` (transaction index, offset of the `ZkDeltaPairs` body, length, source) -
/// source 0: the transaction's `delta`, 1: the record's `state_delta`, 2 (length 0): neither (`StateNotGiven`).  The spans re-slice to the input of
/// `bzk_state_update_chain_bincode`; the claims are each transaction's last `next_state`.
pub fn contract_delta_spans(bytes: &[u8], n: usize, with_delta: bool, contract_id: ContractId) -> Result<Vec<(u64, u64, u64, u64)>, GpuError> {
    let id: ZkScalar = contract_id.into();
    let form: u32 = if with_delta { 1 } else { 0 }; // BZK_L1_FORM_TX_AND_DELTA / BZK_L1_FORM_TX
    let mut found = 0u64;
    let mut spans: Vec<u64> = Vec::new();
    for _ in 0..2 {
        let st = unsafe {
            sys::bzk_l1_tx_deltas(bytes.as_ptr(), bytes.len() as u64, n as u64, form, scalars_ptr(std::slice::from_ref(&id)), spans.as_mut_ptr(),
                                  (spans.len() / 4) as u64, &mut found)
        };
        if st == sys::BZK_E_ARG {
            let why = unsafe { CStr::from_ptr(sys::bzk_mpn_work_last_error()).to_string_lossy().into_owned() };
            return Err(GpuError::Status(st, why));
        }
        check(ptr::null_mut(), st)?;
        if spans.len() as u64 >= 4 * found {
            break;
        }
        spans = vec![0u64; 4 * found as usize];
    }
    Ok(spans.chunks_exact(4).take(found as usize).map(|s| (s[0], s[1], s[2], s[3])).collect())
}
