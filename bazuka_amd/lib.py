"""ctypes binding of libbzk.so - mirrors include/bzk.h one to one."""
from __future__ import annotations

import collections
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BZK_LIBBZK: another build of the same library (A/B runs of compile-time switches: the gitignored pattern bazuka_amd/libbzk.so.* travels to the GPU box)
LIB_PATH = os.environ.get("BZK_LIBBZK") or os.path.join(_HERE, "libbzk.so")

BZK_F_CANONICAL = 1
BZK_F_DEDUP = 2
BZK_F_THROUGHPUT = 4
BZK_PROVE_CHECK_SAT = 1    # bzk_groth16_prove_witness: one product per row decides satisfaction before a proof is written
BZK_SYNTH_DEFER = 2        # bzk_mpn_work_synthesize's record_matrices: the hash-dependent values left to the device
BZK_SYNTH_DEFER_SIG = 4    # ... and the EdDSA gadget's ladders
L1_FORM_TX = 0             # bzk_l1_tx_verify_batch: the records are bincode(Transaction)
L1_FORM_TX_AND_DELTA = 1   # ... bincode(TransactionAndDelta)


def _flags(canonical=False, dedup=False, throughput=False) -> int:
    return (BZK_F_CANONICAL if canonical else 0) | (BZK_F_DEDUP if dedup else 0) | (BZK_F_THROUGHPUT if throughput else 0)


_lib = None

# name -> (restype, argtypes); must list EVERY symbol declared in include/bzk.h
_vp, _u8p, _u32, _u64, _i32 = C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint64, C.c_int32
SIGNATURES = {
    "bzk_ctx_create": (_i32, [_i32, _vp, C.POINTER(_vp)]),
    "bzk_ctx_destroy": (None, [_vp]),
    "bzk_sync": (_i32, [_vp]),
    "bzk_strerror": (C.c_char_p, [_i32]),
    "bzk_last_error": (C.c_char_p, [_vp]),
    "bzk_last_refusal": (_i32, [_vp]),
    "bzk_abi_version": (_u32, []),
    "bzk_dev_alloc": (_i32, [_vp, _u64, C.POINTER(_vp)]),
    "bzk_dev_free": (_i32, [_vp, _vp]),
    "bzk_ctx_trim": (_i32, [_vp, C.POINTER(_u64)]),
    "bzk_h2d": (_i32, [_vp, _vp, _vp, _u64]),
    "bzk_d2h": (_i32, [_vp, _vp, _vp, _u64]),
    "bzk_prof_enable": (_i32, [_vp, _i32]),
    "bzk_prof_filter": (_i32, [_vp, C.c_char_p]),
    "bzk_prof_reset": (_i32, [_vp]),
    "bzk_prof_query": (_i32, [_vp, C.c_char_p, C.POINTER(_u64), C.POINTER(C.c_double)]),
    "bzk_prof_dump": (_i32, [_vp, _vp, _u64]),
    "bzk_poseidon_batch": (_i32, [_vp, _vp, _u32, _u64, _vp]),
    "bzk_poseidon_batch_dev": (_i32, [_vp, _vp, _u32, _u64, _vp]),
    "bzk_jubjub_verify_batch": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_jubjub_verify_batch_dev": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_jubjub_decompress_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bzk_jubjub_decompress_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bzk_jubjub_verify_batch_compressed": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_jubjub_verify_batch_compressed_dev": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_mpn_tx_verify_batch": (_i32, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "bzk_jubjub_keys_batch": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_jubjub_keys_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_jubjub_sign_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bzk_jubjub_sign_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bzk_mpn_txs_sign": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "bzk_mpn_withdraws_sign": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "bzk_sha3_256_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bzk_sha3_256_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bzk_mpn_withdraw_verify_batch": (_i32, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "bzk_sha512_batch": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_sha512_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_ed25519_verify_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_ed25519_verify_batch_dev": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_mpn_deposit_verify_batch": (_i32, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "bzk_mpn_set_wire_flags": (_i32, [C.c_uint32]),
    "bzk_l1_tx_verify_batch": (_i32, [_vp, _vp, _u64, _u64, C.c_uint32, _vp, _vp]),
    "bzk_ed25519_keys_batch": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_ed25519_keys_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_ed25519_sign_batch": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_ed25519_sign_batch_dev": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_mpn_deposits_sign": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp]),
    "bzk_l1_txs_sign": (_i32, [_vp, _vp, _vp, _u64, _u64, C.c_uint32, _vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_sha3_merkle_roots": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "bzk_sha3_merkle_roots_dev": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp]),
    "bzk_block_bodies_check": (_i32, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp]),
    "bzk_contract_updates_check": (_i32, [_vp, _vp, _vp, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    "bzk_l1_tx_updates": (_i32, [_vp, _u64, _u64, C.c_uint32, _vp, _vp, _u64, _vp]),
    "bzk_l1_tx_deltas": (_i32, [_vp, _u64, _u64, C.c_uint32, _vp, _vp, _u64, _vp]),
    "bzk_merkle4_root": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "bzk_merkle4_root_dev": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "bzk_state_compress": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "bzk_state_compress_bincode": (_i32, [_vp, _vp, _u64, _vp, _u64, _vp]),
    "bzk_state_model_default": (_i32, [_vp, _u64, _vp]),
    "bzk_state_create": (_i32, [_vp, _vp, _u64, C.POINTER(_vp)]),
    "bzk_state_free": (None, [_vp]),
    "bzk_state_update": (_i32, [_vp, _vp, _vp, _vp, _u64, _u64, _vp, C.POINTER(_u64), _vp]),
    "bzk_state_update_bincode": (_i32, [_vp, _vp, _u64, _u64, _vp]),
    "bzk_state_update_chain": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, C.POINTER(_u64), _vp]),
    "bzk_state_update_chain_bincode": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, C.POINTER(_u64)]),
    "bzk_state_root": (_i32, [_vp, _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "bzk_state_get": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_state_prove": (_i32, [_vp, _vp, _u64, _vp, _u64, _vp, C.POINTER(_u32)]),
    "bzk_state_stats": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "bzk_ntt": (_i32, [_vp, _vp, _u32, _i32, _i32]),
    "bzk_ntt_dev": (_i32, [_vp, _vp, _u32, _i32, _i32]),
    "bzk_msm_g1": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_msm_g1_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_msm_g2": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_msm_g2_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_msm_window_count": (_u32, [_u64]),
    "bzk_msm_g1_windows_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    "bzk_msm_g2_windows_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    "bzk_g1_sum": (_i32, [_vp, _u32, _vp]),
    "bzk_g2_sum": (_i32, [_vp, _u32, _vp]),
    "bzk_params_load": (_i32, [_vp, _vp, C.POINTER(_vp)]),
    "bzk_params_free": (None, [_vp, _vp]),
    "bzk_params_slot": (_i32, [_vp, _vp, C.POINTER(_vp)]),
    "bzk_params_h_table": (_i32, [_vp, _vp, _i32]),
    "bzk_params_resident_info": (_i32, [_vp, C.POINTER(_u32), C.POINTER(_u64), C.POINTER(_u64)]),
    "bzk_groth16_prove": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "bzk_groth16_prove_r1cs": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "bzk_r1cs_stage": (_i32, [_vp, _vp, C.POINTER(_vp)]),
    "bzk_staged_wait": (_i32, [_vp]),
    "bzk_staged_free": (None, [_vp]),
    "bzk_staged_read": (_i32, [_vp, _i32, _vp, _u64, C.POINTER(_u64)]),
    "bzk_groth16_prove_staged": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "bzk_r1cs_mats_load": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, C.POINTER(_vp)]),
    "bzk_r1cs_mats_from_r1cs": (_i32, [_vp, _vp, C.POINTER(_vp)]),
    "bzk_r1cs_mats_free": (None, [_vp, _vp]),
    "bzk_r1cs_mats_info": (_i32, [_vp, C.POINTER(_u64)]),
    "bzk_r1cs_eval": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, C.POINTER(C.c_int64)]),
    "bzk_r1cs_eval_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64]),
    "bzk_groth16_prove_witness": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _u32, _vp]),
    "bzk_bellman_params_info": (_i32, [_vp, _u64, C.POINTER(_u64)]),
    "bzk_bellman_params_decode": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "bzk_bellman_params_encode": (_i32, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "bzk_params_load_bellman": (_i32, [_vp, _vp, _u64, _u32, _u32, _vp, _vp, C.POINTER(_vp), _vp, _u64]),
    "bzk_bellman_params_check": (_i32, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "bzk_params_load_bellman_checked": (_i32, [_vp, _vp, _u64, _u32, _u32, _vp, _vp, C.POINTER(_vp), _vp, _u64, C.POINTER(_u64)]),
    "bzk_groth16_verify": (_i32, [_vp, _u64, _vp, _u32, _vp]),
    "bzk_groth16_verify_batch": (_i32, [_vp, _vp, _u64, _vp, _u32, _vp, _u64, _vp]),
    "bzk_groth16_verify_batch_dev": (_i32, [_vp, _vp, _u64, _vp, _u32, _vp, _u64, _vp]),
    "bzk_groth16_verify_batch_keys": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_groth16_verify_groups_dev": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bzk_g1_subgroup_check_batch": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_g1_subgroup_check_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_g2_subgroup_check_batch": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_g2_subgroup_check_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_params_read": (_i32, [_vp, _vp, _i32, _vp, _u64, C.POINTER(_u64)]),
    "bzk_groth16_setup": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, C.POINTER(_vp), _vp, _u64]),
    "bzk_g1_scale_batch": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "bzk_g1_scale_batch_dev": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "bzk_params_rekey": (_i32, [_vp, _vp, _vp, C.POINTER(_vp), _vp]),
    "bzk_bellman_params_rekey": (_i32, [_vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(_u64)]),
    "bzk_bellman_params_rekey_check": (_i32, [_vp, _vp, _u64, _vp, _u64, _vp, C.POINTER(_u64)]),
    "bzk_g1_mul_batch": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    "bzk_g1_mul_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    "bzk_g2_mul_batch": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    "bzk_g2_mul_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    "bzk_g1_mul_powers": (_i32, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "bzk_g1_mul_powers_dev": (_i32, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "bzk_g2_mul_powers": (_i32, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "bzk_g2_mul_powers_dev": (_i32, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "bzk_ptau_size": (_u64, [_u32]),
    "bzk_ptau_init": (_i32, [_u32, _vp, _u64]),
    "bzk_ptau_contribute": (_i32, [_vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "bzk_ptau_check": (_i32, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "bzk_groth16_h_dev": (_i32, [_vp, _vp, _vp, _vp, _u32]),
    "bzk_mpn_create": (_i32, [_u32, _u32, C.POINTER(_vp)]),
    "bzk_mpn_destroy": (None, [_vp]),
    "bzk_mpn_set_height": (_i32, [_vp, _u64]),
    "bzk_mpn_set_threads": (_i32, [_vp, _i32]),
    "bzk_host_default_threads": (_i32, []),
    "bzk_mpn_set_device": (_i32, [_vp, _vp]),
    "bzk_mpn_add_account": (_i32, [_vp, _u64, _vp, _u32, _vp, _u64, _vp]),
    "bzk_mpn_add_key": (_i32, [_vp, _u64, _vp, _u32]),
    "bzk_mpn_root": (_i32, [_vp, _vp]),
    "bzk_mpn_push_tx": (_i32, [_vp, _u64, _u64, _vp, _u64, _vp, _u64]),
    "bzk_tree4_create": (_i32, [_vp, _u32, _vp, _vp, C.POINTER(_vp)]),
    "bzk_tree4_free": (None, [_vp, _vp]),
    "bzk_tree4_root": (_i32, [_vp, _vp, _vp]),
    "bzk_tree4_update": (_i32, [_vp, _vp, _vp, _vp, _u64]),
    "bzk_tree4_prove": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_tree4_node": (_i32, [_vp, _vp, _u32, _u64, _vp]),
    "bzk_mpn_state_compress_dev": (_i32, [_vp, _u32, _u32, _vp, _vp, _vp]),
    "bzk_mpn_tree_create": (_i32, [_vp, _u32, _u32, _u64, C.POINTER(_vp)]),
    "bzk_mpn_tree_free": (None, [_vp, _vp]),
    "bzk_mpn_tree_root": (_i32, [_vp, _vp, _vp]),
    "bzk_mpn_tree_accounts": (_u64, [_vp]),
    "bzk_mpn_tree_set_accounts": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64]),
    "bzk_mpn_tree_get_accounts": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_mpn_tree_prove": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "bzk_mpn_tree_prove_token": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp]),
    "bzk_mpn_push_txs": (_i32, [_vp, _vp, _u64, _u64, _vp, C.POINTER(_u64)]),
    "bzk_mpn_push_withdraws": (_i32, [_vp, _vp, _u64, _u64, _vp, C.POINTER(_u64)]),
    "bzk_mpn_push_deposits": (_i32, [_vp, _vp, _u64, _u64, _vp, C.POINTER(_u64)]),
    "bzk_mpn_push_deposit": (_i32, [_vp, _u64, _vp, _u64]),
    "bzk_mpn_push_withdraw": (_i32, [_vp, _u64, _vp, _u64, _vp, _u64, _vp]),
    "bzk_mpn_push_withdraw_signed": (_i32, [_vp, _vp, _u32, _vp, _u64, _vp, _u64, _vp, _vp]),
    "bzk_mpn_deposit_synthesize": (_i32, [_vp, _u32, _vp, _i32, C.POINTER(_vp)]),
    "bzk_mpn_withdraw_synthesize": (_i32, [_vp, _u32, _vp, _i32, C.POINTER(_vp)]),
    "bzk_mpn_circuit_empty": (_i32, [_i32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _i32, C.POINTER(_vp)]),
    "bzk_mpn_update_synthesize": (_i32, [_vp, _u32, _vp, _vp, _i32, C.POINTER(_vp)]),
    "bzk_mpn_update_empty": (_i32, [_u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _i32, C.POINTER(_vp)]),
    "bzk_r1cs_info": (_i32, [_vp, C.POINTER(_u64)]),
    "bzk_r1cs_defer_info": (_i32, [_vp, C.POINTER(_u64)]),
    "bzk_r1cs_fill_host": (_i32, [_vp]),
    "bzk_r1cs_defer_schedule_info": (_i32, [_vp, C.POINTER(_u64)]),
    "bzk_mpn_set_defer": (_i32, [_vp, _i32]),
    "bzk_mpn_set_defer_sig": (_i32, [_vp, _i32]),
    "bzk_r1cs_data": (_vp, [_vp, _i32, C.POINTER(_u64)]),
    "bzk_r1cs_free": (None, [_vp]),
    "bzk_host_poseidon": (_i32, [_vp, _u32, _vp]),
    "bzk_host_sha3_256": (_i32, [_vp, _u64, _vp]),
    "bzk_host_sha512": (_i32, [_vp, _u64, _vp]),
    "bzk_host_ed25519_verify": (_i32, [_vp, _vp, _u64, _vp]),
    "bzk_host_ed25519_keys": (_i32, [_vp, _u64, _vp]),
    "bzk_host_ed25519_sign": (_i32, [_vp, _vp, _u64, _vp]),
    "bzk_host_jubjub_keys": (_i32, [_vp, _u32, _vp]),
    "bzk_host_jubjub_sign": (_i32, [_vp, _vp, _vp]),
    "bzk_host_jubjub_verify": (_i32, [_vp, _vp, _vp]),
    "bzk_host_jubjub_decompress": (_i32, [_vp, _i32, _vp]),
    "bzk_msm_g1_table_build": (_i32, [_vp, _vp, _u64, C.POINTER(_vp)]),
    "bzk_msm_g2_table_build": (_i32, [_vp, _vp, _u64, C.POINTER(_vp)]),
    "bzk_msm_g1_table_build_c": (_i32, [_vp, _vp, _u64, _u32, C.POINTER(_vp)]),
    "bzk_msm_g1_table_build_levels": (_i32, [_vp, _vp, _u64, _u32, C.POINTER(_vp)]),
    "bzk_msm_g2_table_build_levels": (_i32, [_vp, _vp, _u64, _u32, C.POINTER(_vp)]),
    "bzk_msm_table_levels": (_u32, [_vp]),
    "bzk_msm_g1_table_run_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_msm_g2_table_run_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_msm_g1_table_windows_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    "bzk_msm_g2_table_windows_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    "bzk_msm_table_window_count": (_u32, [_vp]),
    "bzk_msm_table_free": (None, [_vp, _vp]),
    "bzk_mpn_work_decode": (_i32, [_vp, _u64, _u32, C.POINTER(_vp), C.POINTER(_u64)]),
    "bzk_mpn_work_last_error": (C.c_char_p, []),
    "bzk_mpn_work_free": (None, [_vp]),
    "bzk_mpn_work_info": (_i32, [_vp, C.POINTER(_u64)]),
    "bzk_mpn_work_scalars": (_i32, [_vp, _vp]),
    "bzk_mpn_work_vk": (_i32, [_vp, _i32, _vp, _u64, C.POINTER(_u64)]),
    "bzk_mpn_work_commitment": (_i32, [_vp, _vp, _vp]),
    "bzk_mpn_work_verify": (_i32, [_vp, _vp, _vp]),
    "bzk_mpn_work_synthesize": (_i32, [_vp, _vp, _vp, _i32, _i32, C.POINTER(_vp)]),
    "bzk_mpn_work_encode": (_i32, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "bzk_mpn_make_work": (_i32, [_vp, _i32, _vp, _u64, C.POINTER(_vp)]),
    "bzk_host_scalar_new": (_i32, [_vp, _u32, _vp]),
    "bzk_zkproof_encode": (_i32, [_vp, _vp]),
    "bzk_zkproof_decode": (_i32, [_vp, _u64, _vp]),
    "bzk_msm_g1_bases_load_dev": (_i32, [_vp, _vp, _u64, C.POINTER(_vp)]),
    "bzk_msm_g2_bases_load_dev": (_i32, [_vp, _vp, _u64, C.POINTER(_vp)]),
    "bzk_msm_bases_free": (None, [_vp, _vp]),
    "bzk_msm_bases_size": (_u64, [_vp]),
    "bzk_msm_bases_info": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_i32), C.POINTER(_u64)]),
    "bzk_msm_bases_table_info": (_i32, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u64)]),
    "bzk_msm_g1_bases_run_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_msm_g2_bases_run_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_msm_g1_bases_windows_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    "bzk_msm_g2_bases_windows_dev": (_i32, [_vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp]),
    "bzk_mg_unique_id": (_i32, [_vp]),
    "bzk_mg_probe": (_i32, [_i32]),
    "bzk_mg_create": (_i32, [C.POINTER(_i32), _i32, _u32, C.POINTER(_vp)]),
    "bzk_mg_create_rank": (_i32, [_i32, _i32, _i32, _vp, _u32, C.POINTER(_vp)]),
    "bzk_mg_destroy": (None, [_vp]),
    "bzk_mg_world": (_i32, [_vp]),
    "bzk_mg_local": (_i32, [_vp]),
    "bzk_mg_rank": (_i32, [_vp]),
    "bzk_mg_exchange": (_u32, [_vp]),
    "bzk_mg_ctx": (_vp, [_vp, _i32]),
    "bzk_mg_stats": (_i32, [_vp, _i32, C.POINTER(C.c_double)]),
    "bzk_mg_last_error": (C.c_char_p, [_vp]),
    "bzk_mg_bases_g1_load": (_i32, [_vp, _vp, _u64, C.POINTER(_vp)]),
    "bzk_mg_bases_g2_load": (_i32, [_vp, _vp, _u64, C.POINTER(_vp)]),
    "bzk_mg_bases_g1_load_dev": (_i32, [_vp, C.POINTER(_vp), _u64, C.POINTER(_vp)]),
    "bzk_mg_bases_g2_load_dev": (_i32, [_vp, C.POINTER(_vp), _u64, C.POINTER(_vp)]),
    "bzk_mg_bases_free": (None, [_vp, _vp]),
    "bzk_mg_msm_g1": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_mg_msm_g2": (_i32, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "bzk_mg_msm_g1_dev": (_i32, [_vp, _vp, C.POINTER(_vp), _u64, _u32, _vp]),
    "bzk_mg_msm_g2_dev": (_i32, [_vp, _vp, C.POINTER(_vp), _u64, _u32, _vp]),
    "bzk_mg_params_load": (_i32, [_vp, _vp, _u32, C.POINTER(_vp)]),
    "bzk_mg_params_free": (None, [_vp, _vp]),
    "bzk_mg_params_slots": (_u32, [_vp]),
    "bzk_mg_params_stats": (_i32, [_vp, C.POINTER(_u64), _u32]),
    "bzk_mg_prove_submit": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "bzk_mg_prove_wait": (_i32, [_vp, _vp, _u64]),
    "bzk_mg_prove": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "bzk_g1_synth_bases_dev": (_i32, [_vp, _u64, _u64, _u64, _vp]),
    "bzk_g2_synth_bases_dev": (_i32, [_vp, _u64, _u64, _u64, _vp]),
}


class ParamsDesc(C.Structure):
    _fields_ = [("n_in", _u32), ("n_aux", _u32), ("log_m", _u32), ("n_a", _u32), ("n_b", _u32), ("vk", _vp), ("h", _vp),
                ("l", _vp), ("a", _vp), ("b_g1", _vp), ("b_g2", _vp), ("a_density", _vp), ("b_density", _vp)]


class CsrDesc(C.Structure):
    _fields_ = [("n_rows", _u64), ("row_ptr", _vp), ("col", _vp), ("val", _vp)]


class Assignment(C.Structure):
    _fields_ = [("z", _vp), ("az", _vp), ("bz", _vp), ("cz", _vp), ("n_rows", _u64), ("n_vars", _u64)]


class WorkConfig(C.Structure):  # bzk_mpn_work_config
    _fields_ = [("log4_deposit_batch", C.c_uint8), ("log4_withdraw_batch", C.c_uint8), ("log4_update_batch", C.c_uint8),
                ("num_update_batches", _u64), ("num_deposit_batches", _u64), ("num_withdraw_batches", _u64),
                ("deposit_vk", _vp), ("deposit_vk_len", _u64), ("withdraw_vk", _vp), ("withdraw_vk_len", _u64),
                ("update_vk", _vp), ("update_vk_len", _u64), ("new_root_state_size", _u64)]


class BzkError(RuntimeError):
    """status: the C ABI's int32 (BZK_E_*; None where the failure is the binding's own)"""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


class ParamsCheckError(BzkError):
    """a point of a proving key failed the checked reader: report = (array 0 vk head .. 6 b_g2, element index, verdict code, 0)"""

    def __init__(self, msg, report):
        super().__init__(msg, -1)
        self.report = report


BZK_E_UNSAT = -4


def load_library():
    """Loads libbzk.so.  Raises (never falls back) when the HIP extension is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BzkError(f"{LIB_PATH} not built - run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _ptr(x):
    """bytes / bytearray / ctypes buffer / int (device pointer) / torch tensor -> void*"""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if isinstance(x, bytes):
        return C.cast(C.c_char_p(x), C.c_void_p)  # the object's own buffer (caller keeps x alive across the call)
    if isinstance(x, bytearray):
        return C.cast((C.c_char * len(x)).from_buffer(x), C.c_void_p)
    if isinstance(x, C.Array):
        return C.cast(C.addressof(x), C.c_void_p)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.cast(x, C.c_void_p)


class Bzk:
    """One context = one GPU + one HIP stream (pass torch's stream handle to share it)."""

    def __init__(self, device: int = 0, stream: int | None = None, handle=None):
        self.lib = load_library()
        self.borrowed = handle is not None
        if handle is not None:  # a context owned by someone else (bzk_mg_ctx): never destroyed from here
            self.h = C.c_void_p(handle) if isinstance(handle, int) else handle
            self.device = device
            return
        h = C.c_void_p()
        st = self.lib.bzk_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(h))
        if st != 0:
            raise BzkError(f"bzk_ctx_create failed: {self.lib.bzk_strerror(st).decode()} (no CPU fallback exists)")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            if not self.borrowed:
                self.lib.bzk_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st: int, what: str):
        if st != 0:
            raise BzkError(f"{what}: {self.lib.bzk_strerror(st).decode()} [{self.lib.bzk_last_error(self.h).decode()}]", st)

    def sync(self):
        self._ck(self.lib.bzk_sync(self.h), "sync")

    def trim(self) -> int:
        """hand the grow-only call workspace back to the device (after a one-off large call); returns the bytes released"""
        n = C.c_uint64(0)
        self._ck(self.lib.bzk_ctx_trim(self.h, C.byref(n)), "ctx_trim")
        return n.value

    def last_refusal(self) -> int:
        """BZK_REFUSE_*: which of the reference's errors the last refused bzk_state_* call stands for"""
        return self.lib.bzk_last_refusal(self.h)

    # ---- profiling
    def prof_filter(self, substr: str | None):
        """event pairs only around launches whose label contains `substr` (None: every launch)"""
        self._ck(self.lib.bzk_prof_filter(self.h, substr.encode() if substr else None), "prof_filter")

    def prof_enable(self, on=True):
        self._ck(self.lib.bzk_prof_enable(self.h, int(on)), "prof_enable")

    def prof_reset(self):
        self._ck(self.lib.bzk_prof_reset(self.h), "prof_reset")

    def prof_query(self, name: str):
        n, ms = C.c_uint64(), C.c_double()
        self._ck(self.lib.bzk_prof_query(self.h, name.encode(), C.byref(n), C.byref(ms)), "prof_query")
        return n.value, ms.value

    def prof_dump(self) -> dict:
        buf = C.create_string_buffer(1 << 16)
        self._ck(self.lib.bzk_prof_dump(self.h, buf, len(buf)), "prof_dump")
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms = line.split()
            out[name] = (int(n), float(ms))
        return out

    # ---- host-pointer (drop-in) forms
    def poseidon_batch(self, inp: bytes, arity: int) -> bytes:
        n = len(inp) // (32 * arity) if arity else 0
        out = C.create_string_buffer(max(32 * n, 1))
        self._ck(self.lib.bzk_poseidon_batch(self.h, _ptr(inp), arity, n, out), "poseidon_batch")
        return out.raw[: 32 * n]

    def jubjub_verify_batch(self, pub_xy: bytes, msg: bytes, sig: bytes) -> bytes:
        """n = len(msg) / 32 signatures (pub_xy n x 64, sig n x 96 = r.x | r.y | s): one verdict byte each, 1 / 0"""
        n = len(msg) // 32
        if len(pub_xy) != 64 * n or len(sig) != 96 * n or len(msg) != 32 * n:
            raise BzkError("jubjub_verify_batch: pub_xy, msg and sig describe different counts")
        out = C.create_string_buffer(max(n, 1))
        self._ck(self.lib.bzk_jubjub_verify_batch(self.h, _ptr(pub_xy), _ptr(msg), _ptr(sig), n, out), "jubjub_verify_batch")
        return out.raw[:n]

    def jubjub_decompress_batch(self, x: bytes, odd: bytes):
        """n = len(odd) compressed keys (x n x 32, odd one byte each): (xy n x 64, ok n bytes); zeros and 0 where a key does not decompress"""
        n = len(odd)
        if len(x) != 32 * n:
            raise BzkError("jubjub_decompress_batch: x and odd describe different counts")
        xy, ok = C.create_string_buffer(max(64 * n, 1)), C.create_string_buffer(max(n, 1))
        self._ck(self.lib.bzk_jubjub_decompress_batch(self.h, _ptr(x), _ptr(odd), n, xy, ok), "jubjub_decompress_batch")
        return xy.raw[: 64 * n], ok.raw[:n]

    def jubjub_verify_batch_compressed(self, pk_x: bytes, pk_odd: bytes, msg: bytes, sig: bytes) -> bytes:
        """jubjub_verify_batch on compressed keys (pk_x n x 32, pk_odd n bytes): decompressed on the device first"""
        n = len(msg) // 32
        if len(pk_x) != 32 * n or len(pk_odd) != n or len(sig) != 96 * n or len(msg) != 32 * n:
            raise BzkError("jubjub_verify_batch_compressed: the arrays describe different counts")
        out = C.create_string_buffer(max(n, 1))
        self._ck(self.lib.bzk_jubjub_verify_batch_compressed(self.h, _ptr(pk_x), _ptr(pk_odd), _ptr(msg), _ptr(sig), n, out),
                 "jubjub_verify_batch_compressed")
        return out.raw[:n]

    def jubjub_keys_batch(self, seeds) -> bytes:
        """JubJub::generate_keys for each of the byte strings in seeds on the device: n x 128 (pub.x | pub.y | randomness | scalar)"""
        return _jubjub_keys_batch(self.h, seeds)

    def jubjub_sign_batch(self, keys: bytes, msg: bytes):
        """n = len(msg) / 32 rows (keys n x 128 as jubjub_keys_batch writes them): (signatures n x 96 = r.x | r.y | s, verdict bytes); a row with
        a field that is not a residue's limbs gets 96 zero bytes and verdict 0"""
        return _jubjub_sign_batch(self.h, keys, msg)

    def mpn_txs_sign(self, keys: bytes, txs: bytes, n: int, want_hash: bool = True):
        """n consecutive bincode(MpnTransaction) and n keys (n x 128): (the records with each signed one's signature replaced, verdict bytes,
        tx hashes n x 32 or None); a malformed record raises"""
        return _mpn_txs_sign(self.h, keys, txs, n, want_hash)

    def mpn_withdraws_sign(self, keys: bytes, txs: bytes, n: int, want_fingerprint: bool = True):
        """n consecutive bincode(MpnWithdraw) and n keys (n x 128): (the records with each signed one's mpn_sig and payment.calldata replaced,
        verdict bytes, payment fingerprints n x 32 or None); a malformed record raises"""
        return _mpn_withdraws_sign(self.h, keys, txs, n, want_fingerprint)

    def mpn_tx_verify_batch(self, txs: bytes, n: int, want_hash: bool = True):
        """n consecutive bincode(MpnTransaction): (verdict bytes, tx hashes n x 32 or None); a malformed record raises"""
        return _mpn_tx_verify_batch(self.h, txs, n, want_hash)

    def sha3_256_batch(self, msgs, want_digest: bool = True, want_scalar: bool = True):
        """SHA3-256 of each of the byte strings in msgs on the device: (digests n x 32 or None, hash_to_scalar n x 32 Montgomery or None)"""
        n = len(msgs)
        off = (_u64 * (n + 1))()
        for i, m in enumerate(msgs):
            off[i + 1] = off[i] + len(m)
        data = b"".join(msgs)
        dig = C.create_string_buffer(max(32 * n, 1)) if want_digest else None
        sc = C.create_string_buffer(max(32 * n, 1)) if want_scalar else None
        self._ck(self.lib.bzk_sha3_256_batch(self.h, _ptr(data) if data else _ptr(b"\0"), off, n, dig, sc), "sha3_256_batch")
        return (dig.raw[: 32 * n] if want_digest else None), (sc.raw[: 32 * n] if want_scalar else None)

    def mpn_withdraw_verify_batch(self, txs: bytes, n: int, want_fingerprint: bool = True):
        """n consecutive bincode(MpnWithdraw): (verdict bytes: bit 0 signature, bit 1 calldata; fingerprints n x 32 or None); a malformed
        record raises"""
        return _mpn_withdraw_verify_batch(self.h, txs, n, want_fingerprint)

    def sha512_batch(self, msgs) -> bytes:
        """SHA-512 of each of the byte strings in msgs on the device: digests n x 64"""
        return _sha512_batch(self.h, msgs)

    def ed25519_verify_batch(self, pks: bytes, msgs, sigs: bytes) -> bytes:
        """Ed25519 (the node's non-strict ed25519-dalek 1 verifier) for len(msgs) signatures: pks n x 32, sigs n x 64; verdict bytes"""
        return _ed25519_verify_batch(self.h, pks, msgs, sigs)

    def groth16_verify_batch(self, vk_bincode: bytes, inputs: bytes, n_inputs: int, proofs: bytes) -> bytes:
        """`groth16_verify` for len(proofs) / 387 proofs of one key, one device lane per proof: inputs n x n_inputs x 32 B Montgomery; verdict bytes"""
        return _groth16_verify_batch(self.h, vk_bincode, inputs, n_inputs, proofs)

    def groth16_verify_batch_keys(self, keys, key_of, inputs: bytes, proofs: bytes) -> bytes:
        """`groth16_verify` for len(proofs) / 387 proofs of SEVERAL keys in one set of launches: keys = [(vk_bincode, n_inputs)], proof i of key
        key_of[i], inputs packed in proof order (32 n_inputs[key_of[i]] bytes each); verdict bytes in the caller's order"""
        return _groth16_verify_batch_keys(self.h, keys, key_of, inputs, proofs)

    def mpn_deposit_verify_batch(self, txs: bytes, n: int, want_address: bool = True):
        """n consecutive bincode(MpnDeposit): (verdict bytes: bit 0 the payment's Ed25519 signature, bit 1 the address decompresses; addresses
        n x 64 or None); a malformed record raises"""
        return _mpn_deposit_verify_batch(self.h, txs, n, want_address)

    def ed25519_keys_batch(self, seeds) -> bytes:
        """Ed25519::generate_keys for each of the byte strings in seeds on the device: n x 64 (secret | public)"""
        return _ed25519_keys_batch(self.h, seeds)

    def ed25519_sign_batch(self, keys: bytes, msgs) -> bytes:
        """len(msgs) rows (keys n x 64 as ed25519_keys_batch writes them): the signatures, n x 64 = R | s"""
        return _ed25519_sign_batch(self.h, keys, msgs)

    def mpn_deposits_sign(self, keys: bytes, txs: bytes, n: int, want_txs: bool = True):
        """n consecutive bincode(MpnDeposit) and n keys (n x 64): (signatures n x 64, verdict bytes, the records with Some(sig) filled in or
        None); a record whose payment.src is not its key's public half keeps verdict 0, a zero signature and its bytes; a malformed record raises"""
        return _mpn_deposits_sign(self.h, keys, txs, n, want_txs)

    def l1_txs_sign(self, keys: bytes, txs: bytes, n: int, form: int = L1_FORM_TX, want_hash: bool = True, want_txs: bool = True):
        """n consecutive bincode(Transaction) / bincode(TransactionAndDelta) and n keys (n x 64): (signatures n x 64, verdict bytes, hashes
        n x 32 or None, the records with Signature::Signed(sig) or None); src None or another key's: verdict 0; a malformed record raises"""
        return _l1_txs_sign(self.h, keys, txs, n, form, want_hash, want_txs)

    def l1_tx_verify_batch(self, txs: bytes, n: int, form: int = L1_FORM_TX, want_hash: bool = True):
        """n consecutive bincode(Transaction) (form L1_FORM_TX) or bincode(TransactionAndDelta) (L1_FORM_TX_AND_DELTA): (verdict bytes of
        Transaction::verify_signature, Transaction::hash n x 32 or None); a malformed record raises"""
        return _l1_tx_verify_batch(self.h, txs, n, form, want_hash)

    def sha3_merkle_roots(self, leaves: bytes, counts, want_nodes: bool = False):
        """MerkleTree::<Sha3Hasher>::new for len(counts) trees whose 32-byte leaves lie one tree after another in leaves: roots m x 32, or
        (roots, all node arrays in heap order) with want_nodes"""
        return _sha3_merkle_roots(self.h, leaves, counts, want_nodes)

    def sha3_merkle_roots_dev(self, leaves, count, m: int, n_leaves: int, roots, nodes=None):
        """device buffers: leaves n_leaves x 32, count m u64; roots m x 32 and (optionally) nodes are written on the context's stream"""
        self._ck(self.lib.bzk_sha3_merkle_roots_dev(self.h, _ptr(leaves), _ptr(count), m, n_leaves, _ptr(roots), _ptr(nodes)),
                 "sha3_merkle_roots_dev")

    def block_bodies_check(self, txs: bytes, counts, want_tx: bool = True):
        """the bodies of len(counts) blocks as bincode(Transaction) back to back, counts[j] per block: (sig_ok m bytes, roots m x 32, tx_ok n
        bytes or None, hashes n x 32 or None); a malformed record raises"""
        return _block_bodies_check(self.h, txs, counts, want_tx)

    def contract_updates_check(self, contract, updates: bytes, counts, height0: int, state0: bytes):
        """`update_contract`'s per-update checks for the ContractUpdates of len(counts) consecutive transactions of one contract (a
        ContractDesc): (BZK_UPD_* bits n bytes, aux_data.state_hash n x 32, commitments n x 32); a malformed record raises"""
        return _contract_updates_check(self.h, contract, updates, counts, height0, state0)

    def merkle4_root(self, leaves: bytes, log4: int, want_nodes: bool = False):
        root = C.create_string_buffer(32)
        nn = (4 ** log4 - 1) // 3
        nodes = C.create_string_buffer(max(32 * nn, 1)) if want_nodes else None
        self._ck(self.lib.bzk_merkle4_root(self.h, _ptr(leaves), log4, root, nodes), "merkle4_root")
        return (root.raw, nodes.raw[: 32 * nn]) if want_nodes else root.raw

    def ntt(self, data: bytes, log_n: int, inverse=False, coset=False) -> bytes:
        buf = C.create_string_buffer(bytes(data), len(data))
        self._ck(self.lib.bzk_ntt(self.h, buf, log_n, int(inverse), int(coset)), "ntt")
        return buf.raw

    def msm_g1(self, bases: bytes, scalars: bytes, canonical=False, dedup=False, throughput=False) -> bytes:
        n = len(scalars) // 32
        out = C.create_string_buffer(97)
        self._ck(self.lib.bzk_msm_g1(self.h, _ptr(bases), _ptr(scalars), n, _flags(canonical, dedup, throughput), out), "msm_g1")
        return out.raw

    def msm_g2(self, bases: bytes, scalars: bytes, canonical=False, dedup=False, throughput=False) -> bytes:
        n = len(scalars) // 32
        out = C.create_string_buffer(193)
        self._ck(self.lib.bzk_msm_g2(self.h, _ptr(bases), _ptr(scalars), n, _flags(canonical, dedup, throughput), out), "msm_g2")
        return out.raw

    # ---- device-pointer forms (x = torch tensor / int device address)
    def poseidon_batch_dev(self, inp, arity: int, n: int, out):
        self._ck(self.lib.bzk_poseidon_batch_dev(self.h, _ptr(inp), arity, n, _ptr(out)), "poseidon_batch_dev")

    def jubjub_verify_batch_dev(self, pub_xy, msg, sig, n: int, ok):
        """device buffers; ok: n verdict bytes, written in stream order"""
        self._ck(self.lib.bzk_jubjub_verify_batch_dev(self.h, _ptr(pub_xy), _ptr(msg), _ptr(sig), n, _ptr(ok)), "jubjub_verify_batch_dev")

    def jubjub_decompress_batch_dev(self, x, odd, n: int, xy, ok):
        """device buffers; xy n x 64 and ok n bytes are written in stream order"""
        self._ck(self.lib.bzk_jubjub_decompress_batch_dev(self.h, _ptr(x), _ptr(odd), n, _ptr(xy), _ptr(ok)), "jubjub_decompress_batch_dev")

    def jubjub_verify_batch_compressed_dev(self, pk_x, pk_odd, msg, sig, n: int, ok):
        self._ck(self.lib.bzk_jubjub_verify_batch_compressed_dev(self.h, _ptr(pk_x), _ptr(pk_odd), _ptr(msg), _ptr(sig), n, _ptr(ok)),
                 "jubjub_verify_batch_compressed_dev")

    def jubjub_keys_batch_dev(self, seeds, off, n: int, keys_out):
        """device tensors: seeds (bytes), off (n + 1 uint64 offsets from 0), keys_out n x 128 bytes; enqueues on the context's stream"""
        self._ck(self.lib.bzk_jubjub_keys_batch_dev(self.h, _ptr(seeds), _ptr(off), n, _ptr(keys_out)), "jubjub_keys_batch_dev")

    def jubjub_sign_batch_dev(self, keys, msg, n: int, sig_out, ok):
        """device tensors: keys n x 128, msg n x 32, sig_out n x 96, ok n bytes; enqueues on the context's stream and leaves keys alone"""
        self._ck(self.lib.bzk_jubjub_sign_batch_dev(self.h, _ptr(keys), _ptr(msg), n, _ptr(sig_out), _ptr(ok)), "jubjub_sign_batch_dev")

    def ed25519_keys_batch_dev(self, seeds, off, n: int, keys_out):
        """device tensors: seeds (bytes), off (n + 1 uint64 offsets from 0), keys_out n x 64 bytes; enqueues on the context's stream"""
        self._ck(self.lib.bzk_ed25519_keys_batch_dev(self.h, _ptr(seeds), _ptr(off), n, _ptr(keys_out)), "ed25519_keys_batch_dev")

    def ed25519_sign_batch_dev(self, keys, msg, off, n: int, sig_out):
        """device tensors: keys n x 64, msg (bytes), off (n + 1 uint64 offsets from 0), sig_out n x 64; enqueues on the context's stream and
        leaves keys and msg alone"""
        self._ck(self.lib.bzk_ed25519_sign_batch_dev(self.h, _ptr(keys), _ptr(msg), _ptr(off), n, _ptr(sig_out)), "ed25519_sign_batch_dev")

    def sha3_256_batch_dev(self, data, off, n: int, digest=None, scalar=None):
        """device buffers: data bytes, off n + 1 u64; digest n x 32 and / or scalar n x 32 are written in stream order"""
        self._ck(self.lib.bzk_sha3_256_batch_dev(self.h, _ptr(data), _ptr(off), n, _ptr(digest), _ptr(scalar)), "sha3_256_batch_dev")

    def sha512_batch_dev(self, data, off, n: int, digest):
        """device buffers: data bytes, off n + 1 u64; digest n x 64 is written in stream order"""
        self._ck(self.lib.bzk_sha512_batch_dev(self.h, _ptr(data), _ptr(off), n, _ptr(digest)), "sha512_batch_dev")

    def ed25519_verify_batch_dev(self, pk, msg, off, sig, n: int, ok):
        """device buffers: pk n x 32, message bytes, off n + 1 u64, sig n x 64; ok n verdict bytes, written in stream order"""
        self._ck(self.lib.bzk_ed25519_verify_batch_dev(self.h, _ptr(pk), _ptr(msg), _ptr(off), _ptr(sig), n, _ptr(ok)), "ed25519_verify_batch_dev")

    def groth16_verify_batch_dev(self, vk_bincode: bytes, inputs, n_inputs: int, proofs, n: int, ok):
        """device buffers: inputs n x n_inputs x 32, proofs n x 387; ok n verdict bytes (the key is host bytes); synchronises"""
        self._ck(self.lib.bzk_groth16_verify_batch_dev(self.h, _ptr(vk_bincode), len(vk_bincode), _ptr(inputs), n_inputs, _ptr(proofs), n, _ptr(ok)),
                 "groth16_verify_batch_dev")

    def groth16_verify_groups_dev(self, keys, counts, inputs, proofs, ok):
        """device buffers, group after group: keys = [(vk_bincode, n_inputs)] (host bytes), group g is counts[g] proofs of keys[g]; inputs, proofs
        (387 each) and the verdict bytes ok each contiguous in group order; synchronises"""
        vks, vk_off, n_inputs = _pack_keys(keys)
        cnt = (C.c_uint64 * max(len(keys), 1))(*counts)
        self._ck(self.lib.bzk_groth16_verify_groups_dev(self.h, len(keys), _ptr(vks) if vks else None, vk_off, n_inputs, cnt, _ptr(inputs), _ptr(proofs),
                                                        _ptr(ok)), "groth16_verify_groups_dev")

    def subgroup_check_batch(self, group: str, pts: bytes, inf: bytes = None) -> bytes:
        """verdict byte per raw point (group "g1": 96 B, "g2": 192 B): 1 in the subgroup, 0 on the curve outside it, 2 not a curve point"""
        return _subgroup_check_batch(self.h, group, pts, inf)

    def subgroup_check_batch_dev(self, group: str, pts, inf, n: int, ok):
        """device buffers: pts n x 96 / 192, inf n flag bytes or None; ok n verdict bytes; synchronises"""
        fn = {"g1": self.lib.bzk_g1_subgroup_check_batch_dev, "g2": self.lib.bzk_g2_subgroup_check_batch_dev}[group]
        self._ck(fn(self.h, _ptr(pts), _ptr(inf) if inf is not None else None, n, _ptr(ok)), "subgroup_check_batch_dev")

    def merkle4_root_dev(self, leaves, log4: int, nodes=None) -> bytes:
        root = C.create_string_buffer(32)
        self._ck(self.lib.bzk_merkle4_root_dev(self.h, _ptr(leaves), log4, root, _ptr(nodes)), "merkle4_root_dev")
        return root.raw

    def ntt_dev(self, data, log_n: int, inverse=False, coset=False):
        self._ck(self.lib.bzk_ntt_dev(self.h, _ptr(data), log_n, int(inverse), int(coset)), "ntt_dev")

    def msm_g1_dev(self, bases, scalars, n: int, canonical=False, dedup=False, throughput=False) -> bytes:
        out = C.create_string_buffer(97)
        self._ck(self.lib.bzk_msm_g1_dev(self.h, _ptr(bases), _ptr(scalars), n, _flags(canonical, dedup, throughput), out), "msm_g1_dev")
        return out.raw

    def msm_g2_dev(self, bases, scalars, n: int, canonical=False, dedup=False, throughput=False) -> bytes:
        out = C.create_string_buffer(193)
        self._ck(self.lib.bzk_msm_g2_dev(self.h, _ptr(bases), _ptr(scalars), n, _flags(canonical, dedup, throughput), out), "msm_g2_dev")
        return out.raw

    # ---- device-resident 4-ary tree
    def tree4_create(self, log4: int, leaves_dev=None, default_leaf: bytes = bytes(32)):
        h = C.c_void_p()
        self._ck(self.lib.bzk_tree4_create(self.h, log4, _ptr(leaves_dev), _ptr(default_leaf), C.byref(h)), "tree4_create")
        return h

    def tree4_free(self, tree):
        self.lib.bzk_tree4_free(self.h, tree)

    def tree4_root(self, tree) -> bytes:
        out = C.create_string_buffer(32)
        self._ck(self.lib.bzk_tree4_root(self.h, tree, out), "tree4_root")
        return out.raw

    def tree4_update(self, tree, indices, leaves: bytes):
        arr = (C.c_uint64 * len(indices))(*indices)
        self._ck(self.lib.bzk_tree4_update(self.h, tree, arr, _ptr(leaves), len(indices)), "tree4_update")

    def tree4_prove(self, tree, indices, log4: int) -> bytes:
        arr = (C.c_uint64 * len(indices))(*indices)
        out = C.create_string_buffer(max(1, len(indices) * log4 * 96))
        self._ck(self.lib.bzk_tree4_prove(self.h, tree, arr, len(indices), out), "tree4_prove")
        return out.raw[: len(indices) * log4 * 96]

    def tree4_node(self, tree, depth: int, index: int) -> bytes:
        out = C.create_string_buffer(32)
        self._ck(self.lib.bzk_tree4_node(self.h, tree, depth, index, out), "tree4_node")
        return out.raw

    def msm_window_count(self, n: int) -> int:
        return self.lib.bzk_msm_window_count(n)

    def msm_g1_windows_dev(self, bases, scalars, n: int, w0: int, w1: int, canonical=False, dedup=False, throughput=False) -> bytes:
        out = C.create_string_buffer(97)
        flags = _flags(canonical, dedup, throughput)
        self._ck(self.lib.bzk_msm_g1_windows_dev(self.h, _ptr(bases), _ptr(scalars), n, flags, w0, w1, out), "msm_g1_windows_dev")
        return out.raw

    def msm_g2_windows_dev(self, bases, scalars, n: int, w0: int, w1: int, canonical=False, dedup=False, throughput=False) -> bytes:
        out = C.create_string_buffer(193)
        flags = _flags(canonical, dedup, throughput)
        self._ck(self.lib.bzk_msm_g2_windows_dev(self.h, _ptr(bases), _ptr(scalars), n, flags, w0, w1, out), "msm_g2_windows_dev")
        return out.raw

    # ---- resident base sets
    def msm_bases_load_dev(self, bases, n: int, g2=False):
        """a static point set converted once into the internal form and kept in HBM (include/bzk.h: resident base sets)"""
        h = C.c_void_p()
        fn = self.lib.bzk_msm_g2_bases_load_dev if g2 else self.lib.bzk_msm_g1_bases_load_dev
        self._ck(fn(self.h, _ptr(bases), n, C.byref(h)), "msm_bases_load_dev")
        return h

    def msm_bases_info(self, handle) -> dict:
        n, forms, nbytes = C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
        self._ck(self.lib.bzk_msm_bases_info(handle, C.byref(n), C.byref(forms), C.byref(nbytes)), "msm_bases_info")
        return {"n": n.value, "forms": forms.value, "device_bytes": nbytes.value}

    def msm_bases_table_info(self, handle) -> dict:
        """the window table a resident G1 set carries for stand-alone calls (include/bzk.h); all zero without one"""
        c, levels, nbytes = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        self._ck(self.lib.bzk_msm_bases_table_info(handle, C.byref(c), C.byref(levels), C.byref(nbytes)), "msm_bases_table_info")
        return {"c": c.value, "levels": levels.value, "table_bytes": nbytes.value}

    def msm_bases_free(self, handle):
        self.lib.bzk_msm_bases_free(self.h, handle)

    def msm_bases_run_dev(self, handle, scalars, n: int, g2=False, canonical=False, dedup=False, throughput=False) -> bytes:
        out = C.create_string_buffer(193 if g2 else 97)
        fn = self.lib.bzk_msm_g2_bases_run_dev if g2 else self.lib.bzk_msm_g1_bases_run_dev
        self._ck(fn(self.h, handle, _ptr(scalars), n, _flags(canonical, dedup, throughput), out), "msm_bases_run_dev")
        return out.raw

    def msm_bases_windows_dev(self, handle, scalars, n: int, w0: int, w1: int, g2=False, canonical=False, dedup=False) -> bytes:
        out = C.create_string_buffer(193 if g2 else 97)
        fn = self.lib.bzk_msm_g2_bases_windows_dev if g2 else self.lib.bzk_msm_g1_bases_windows_dev
        self._ck(fn(self.h, handle, _ptr(scalars), n, _flags(canonical, dedup), w0, w1, out), "msm_bases_windows_dev")
        return out.raw

    def msm_table_build_c(self, bases, n: int, c: int):
        """full G1 table with an explicit window size"""
        h = C.c_void_p()
        self._ck(self.lib.bzk_msm_g1_table_build_c(self.h, _ptr(bases), n, c, C.byref(h)), "msm_table_build_c")
        return h

    def msm_table_build(self, bases, n: int, g2=False, levels: int = 0):
        """levels = 0: full table (one level per window); levels = L: folded table (see include/bzk.h)"""
        h = C.c_void_p()
        if levels:
            fn = self.lib.bzk_msm_g2_table_build_levels if g2 else self.lib.bzk_msm_g1_table_build_levels
            self._ck(fn(self.h, _ptr(bases), n, levels, C.byref(h)), "msm_table_build_levels")
        else:
            fn = self.lib.bzk_msm_g2_table_build if g2 else self.lib.bzk_msm_g1_table_build
            self._ck(fn(self.h, _ptr(bases), n, C.byref(h)), "msm_table_build")
        return h

    def msm_table_levels(self, table) -> int:
        return self.lib.bzk_msm_table_levels(table)

    def msm_table_run_dev(self, table, scalars, n: int, g2=False, canonical=False, throughput=False) -> bytes:
        out = C.create_string_buffer(193 if g2 else 97)
        fn = self.lib.bzk_msm_g2_table_run_dev if g2 else self.lib.bzk_msm_g1_table_run_dev
        self._ck(fn(self.h, table, _ptr(scalars), n, _flags(canonical, False, throughput), out), "msm_table_run")
        return out.raw

    def msm_table_windows_dev(self, table, scalars, n: int, w0: int, w1: int, g2=False, canonical=False) -> bytes:
        out = C.create_string_buffer(193 if g2 else 97)
        fn = self.lib.bzk_msm_g2_table_windows_dev if g2 else self.lib.bzk_msm_g1_table_windows_dev
        self._ck(fn(self.h, table, _ptr(scalars), n, BZK_F_CANONICAL if canonical else 0, w0, w1, out), "msm_table_windows")
        return out.raw

    def msm_table_window_count(self, table) -> int:
        return self.lib.bzk_msm_table_window_count(table)

    def msm_table_free(self, table):
        self.lib.bzk_msm_table_free(self.h, table)

    def g1_sum(self, packed: bytes) -> bytes:
        out = C.create_string_buffer(97)
        self._ck(self.lib.bzk_g1_sum(_ptr(packed), len(packed) // 97, out), "g1_sum")
        return out.raw

    def g2_sum(self, packed: bytes) -> bytes:
        out = C.create_string_buffer(193)
        self._ck(self.lib.bzk_g2_sum(_ptr(packed), len(packed) // 193, out), "g2_sum")
        return out.raw

    # ---- general `ZkStateModel::compress`
    def state_compress(self, model_bincode: bytes, pairs):
        """pairs: iterable of (locator tuple of ints, 32-byte Montgomery scalar) -> (state_hash 32 B, state_size)"""
        pairs = list(pairs)
        off, loc = [0], []
        for l, _ in pairs:
            loc.extend(l)
            off.append(len(loc))
        o = (_u64 * len(off))(*off)
        lo = (_u64 * max(1, len(loc)))(*loc)
        vals = b"".join(v for _, v in pairs)
        out, size = C.create_string_buffer(32), _u64()
        self._ck(self.lib.bzk_state_compress(self.h, _ptr(model_bincode), len(model_bincode), o, lo, _ptr(vals), len(pairs), out, C.byref(size)),
                 "state_compress")
        return out.raw, size.value

    def state_compress_bincode(self, model_bincode: bytes, pairs_bincode: bytes) -> bytes:
        out = C.create_string_buffer(40)
        self._ck(self.lib.bzk_state_compress_bincode(self.h, _ptr(model_bincode), len(model_bincode), _ptr(pairs_bincode), len(pairs_bincode), out),
                 "state_compress_bincode")
        return out.raw

    # ---- device-resident MPN account state
    def mpn_state_compress_dev(self, log4_tree: int, log4_token_tree: int, cells, tokens) -> bytes:
        """root of a dense MPN-shaped state in device memory: cells = 4^L x 4 scalars, tokens = 4^L x 4^T x 2 scalars"""
        out = C.create_string_buffer(32)
        self._ck(self.lib.bzk_mpn_state_compress_dev(self.h, log4_tree, log4_token_tree, _ptr(cells), _ptr(tokens), out), "mpn_state_compress_dev")
        return out.raw

    def mpn_tree_create(self, log4_tree: int, log4_token_tree: int, capacity: int):
        h = C.c_void_p()
        self._ck(self.lib.bzk_mpn_tree_create(self.h, log4_tree, log4_token_tree, capacity, C.byref(h)), "mpn_tree_create")
        return h

    def mpn_tree_free(self, tree):
        self.lib.bzk_mpn_tree_free(self.h, tree)

    def mpn_tree_root(self, tree) -> bytes:
        out = C.create_string_buffer(32)
        self._ck(self.lib.bzk_mpn_tree_root(self.h, tree, out), "mpn_tree_root")
        return out.raw

    def mpn_tree_set_accounts(self, tree, accounts):
        """accounts: list of (index, (nonce, wnonce, x, y) as 4 x 32 B Montgomery, {token slot: (token_id 32 B, balance 32 B)})"""
        n = len(accounts)
        idx = (_u64 * max(1, n))(*[a[0] for a in accounts])
        cells = b"".join(b"".join(a[1]) for a in accounts)
        off, tix, tv = [0], [], []
        for a in accounts:
            for slot, (tid, bal) in a[2].items():
                tix.append(slot)
                tv.append(tid + bal)
            off.append(len(tix))
        offs = (_u64 * (n + 1))(*off)
        tixs = (_u64 * max(1, len(tix)))(*tix)
        tvb = b"".join(tv)
        self._ck(self.lib.bzk_mpn_tree_set_accounts(self.h, tree, idx, _ptr(cells), offs, tixs, _ptr(tvb), n), "mpn_tree_set_accounts")

    def mpn_tree_get_accounts(self, tree, indices, log4_token_tree: int) -> list:
        """per account: dict(cells = 4 scalars, tokens_root, tokens = {slot: (token_id, balance)} for non-zero token ids)"""
        n, ts = len(indices), 4 ** log4_token_tree
        rec = 5 + 2 * ts
        out = C.create_string_buffer(max(1, n * rec * 32))
        self._ck(self.lib.bzk_mpn_tree_get_accounts(self.h, tree, (_u64 * max(1, n))(*indices), n, out), "mpn_tree_get_accounts")
        res = []
        raw = out.raw  # ONE copy of the buffer (`.raw` copies on every access)
        for a in range(n):
            sc = [raw[32 * (a * rec + j):32 * (a * rec + j + 1)] for j in range(rec)]
            toks = {i: (sc[5 + 2 * i], sc[6 + 2 * i]) for i in range(ts) if sc[5 + 2 * i] != bytes(32)}
            res.append({"cells": sc[:4], "tokens_root": sc[4], "tokens": toks})
        return res

    def mpn_tree_prove(self, tree, indices, log4_tree: int) -> bytes:
        n = len(indices)
        out = C.create_string_buffer(max(1, n * log4_tree * 96))
        self._ck(self.lib.bzk_mpn_tree_prove(self.h, tree, (_u64 * max(1, n))(*indices), n, out), "mpn_tree_prove")
        return out.raw[: n * log4_tree * 96]

    def mpn_tree_prove_token(self, tree, accounts, slots, log4_token_tree: int) -> bytes:
        n = len(accounts)
        out = C.create_string_buffer(max(1, n * log4_token_tree * 96))
        self._ck(self.lib.bzk_mpn_tree_prove_token(self.h, tree, (_u64 * max(1, n))(*accounts), (_u64 * max(1, n))(*slots), n, out),
                 "mpn_tree_prove_token")
        return out.raw[: n * log4_token_tree * 96]

    # ---- Groth16
    def params_load(self, params: dict):
        """params: dict with n_in, n_aux, log_m, n_a, n_b and byte strings vk(870), h, l, a, b_g1, b_g2,
        a_density, b_density (the layout oracle.coracle.groth16_setup produces)."""
        keep = {k: C.create_string_buffer(bytes(params[k]), max(1, len(params[k])))
                for k in ("vk", "h", "l", "a", "b_g1", "b_g2", "a_density", "b_density")}
        d = ParamsDesc(params["n_in"], params["n_aux"], params["log_m"], params["n_a"], params["n_b"],
                       *[C.cast(keep[k], C.c_void_p) for k in ("vk", "h", "l", "a", "b_g1", "b_g2", "a_density", "b_density")])
        h = C.c_void_p()
        self._ck(self.lib.bzk_params_load(self.h, C.byref(d), C.byref(h)), "params_load")
        return h

    def params_load_bellman(self, blob: bytes, n_in: int, n_aux: int, a_density: bytes, b_density: bytes):
        """bellman `Parameters::write` bytes + the circuit shape's density maps -> (params handle, bincode Groth16VerifyingKey)"""
        h = C.c_void_p()
        vk = C.create_string_buffer(878 + 97 * n_in)
        self._ck(self.lib.bzk_params_load_bellman(self.h, _ptr(blob), len(blob), n_in, n_aux, _ptr(a_density), _ptr(b_density), C.byref(h),
                                                  vk, len(vk)), "params_load_bellman")
        return h, vk.raw

    def params_load_bellman_checked(self, blob: bytes, n_in: int, n_aux: int, a_density: bytes, b_density: bytes):
        """params_load_bellman with the subgroup check of every point (`Parameters::read(.., checked = true)`): a failed point raises
        ParamsCheckError, whose `report` is (array, index, verdict code, 0); no handle is left"""
        h = C.c_void_p()
        vk = C.create_string_buffer(878 + 97 * n_in)
        report = (C.c_uint64 * 4)()
        st = self.lib.bzk_params_load_bellman_checked(self.h, _ptr(blob), len(blob), n_in, n_aux, _ptr(a_density), _ptr(b_density), C.byref(h),
                                                      vk, len(vk), report)
        if st == -1 and not h.value:
            raise ParamsCheckError("params_load_bellman_checked: " + self.lib.bzk_last_error(self.h).decode(), tuple(report))
        self._ck(st, "params_load_bellman_checked")
        return h, vk.raw

    def bellman_params_check(self, blob: bytes):
        """(verdict, report): `Parameters::read(.., checked = true)` as a verdict, the queries on the device"""
        return _bellman_params_check(self.h, blob)

    def params_free(self, ph):
        self.lib.bzk_params_free(self.h, ph)

    def params_slot(self, ph):
        """another prover slot over the same device-resident CRS (own scratch): one ctx + one slot per concurrent prover thread"""
        h = C.c_void_p()
        self._ck(self.lib.bzk_params_slot(self.h, ph, C.byref(h)), "params_slot")
        return h

    def params_h_table(self, ph, on: bool):
        self._ck(self.lib.bzk_params_h_table(self.h, ph, int(on)), "params_h_table")

    def params_resident_info(self, ph) -> dict:
        """the resident query sets a parameter set holds once prepared (include/bzk.h)"""
        k, nbytes, tab = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.bzk_params_resident_info(ph, C.byref(k), C.byref(nbytes), C.byref(tab)), "params_resident_info")
        return {"sets": k.value, "device_bytes": nbytes.value, "table_bytes": tab.value}

    def groth16_prove(self, ph, z, az, bz, cz, r: bytes, s: bytes) -> bytes:
        """z / az / bz / cz: bytes or zero-copy ctypes views (R1cs.raw) - passed by address, never copied here."""
        keep = [x if not isinstance(x, bytearray) else bytes(x) for x in (z, az, bz, cz)]
        if not (len(az) == len(bz) == len(cz)) or len(az) % 32 or len(z) % 32:
            raise BzkError(f"groth16_prove: z / az / bz / cz lengths {len(z)}, {len(az)}, {len(bz)}, {len(cz)}")
        asg = Assignment(*[_ptr(x) for x in keep], len(az) // 32, len(z) // 32)  # libbzk checks n_vars against the params
        out = C.create_string_buffer(387)
        self._ck(self.lib.bzk_groth16_prove(self.h, ph, C.byref(asg), _ptr(r), _ptr(s), out), "groth16_prove")
        return out.raw

    def groth16_prove_r1cs(self, ph, r1cs, r: bytes, s: bytes) -> bytes:
        """the same over an R1cs of the host generator; an instance synthesized with MpnWorld.set_defer(True) is completed on the device first"""
        out = C.create_string_buffer(387)
        self._ck(self.lib.bzk_groth16_prove_r1cs(self.h, ph, r1cs.h, _ptr(r), _ptr(s), out), "groth16_prove_r1cs")
        return out.raw

    def r1cs_stage(self, r1cs):
        """the instance's arrays into HBM on THIS context's stream + its deferred-value program behind them; returns at once (a staged handle).
        Keep `r1cs` alive until staged_wait / a prove call on the handle has returned."""
        h = C.c_void_p()
        self._ck(self.lib.bzk_r1cs_stage(self.h, r1cs.h, C.byref(h)), "r1cs_stage")
        return h

    def staged_wait(self, staged):
        self._ck(self.lib.bzk_staged_wait(staged), "staged_wait")

    def staged_free(self, staged):
        self.lib.bzk_staged_free(staged)

    def staged_read(self, staged, which: int) -> bytes:
        """one staged array (0 z, 1 az, 2 bz, 3 cz) as the DEVICE left it after the uploads and the deferred-value program"""
        n = _u64()
        self._ck(self.lib.bzk_staged_read(staged, which, None, 0, C.byref(n)), "staged_read")
        buf = (C.c_uint8 * n.value)()
        self._ck(self.lib.bzk_staged_read(staged, which, buf, n.value, None), "staged_read")
        return bytes(buf)

    def groth16_prove_staged(self, ph, staged, r: bytes, s: bytes) -> bytes:
        out = C.create_string_buffer(387)
        self._ck(self.lib.bzk_groth16_prove_staged(self.h, ph, staged, _ptr(r), _ptr(s), out), "groth16_prove_staged")
        return out.raw

    # ---- proving from the witness alone: the circuit's matrices resident, A.z / B.z / C.z on the device (include/bzk.h)
    def r1cs_mats_load(self, csr_abc, n_in: int, n_aux: int):
        """csr_abc as groth16_setup takes it; the matrices become resident on this context's device.  Returns the handle."""
        return _r1cs_mats_load(self.h, csr_abc, n_in, n_aux)

    def r1cs_mats_from(self, r1cs):
        """the same from an R1cs synthesized with record_matrices"""
        return _r1cs_mats_from(self.h, r1cs)

    def r1cs_mats_free(self, mh):
        self.lib.bzk_r1cs_mats_free(self.h, mh)

    def r1cs_mats_info(self, mh) -> dict:
        return r1cs_mats_info(mh)

    def r1cs_eval(self, mh, z, want_unsat: bool = False):
        """(az, bz, cz) of the host witness z on the device; with want_unsat also the first unsatisfied row (-1: none)"""
        return _r1cs_eval(self.h, mh, z, want_unsat)

    def r1cs_eval_dev(self, mh, z, n_vars: int, az, bz, cz, pad_rows: int):
        """device buffers (tensors / pointers; an output may be None), enqueued on the context's stream; rows n_rows .. pad_rows are zeroed"""
        self._ck(self.lib.bzk_r1cs_eval_dev(self.h, mh, _ptr(z), n_vars, _ptr(az), _ptr(bz), _ptr(cz), pad_rows), "r1cs_eval_dev")

    def groth16_prove_witness(self, ph, mh, z, r: bytes, s: bytes, check: bool = False, out=None) -> bytes:
        """groth16_prove from z alone: the evaluations come from the resident matrices `mh`.  check: BZK_PROVE_CHECK_SAT - an unsatisfied
        witness raises (status BZK_E_UNSAT, the row in the message) and nothing is written to `out` (a 387-byte ctypes buffer, optional)."""
        zz = bytes(z) if isinstance(z, bytearray) else z
        out = C.create_string_buffer(387) if out is None else out
        self._ck(self.lib.bzk_groth16_prove_witness(self.h, ph, mh, _ptr(zz), len(zz) // 32, _ptr(r), _ptr(s),
                                                    BZK_PROVE_CHECK_SAT if check else 0, out), "groth16_prove_witness")
        return out.raw

    def params_read(self, ph, which: int) -> bytes:
        n = _u64()
        self._ck(self.lib.bzk_params_read(self.h, ph, which, None, 0, C.byref(n)), "params_read")
        buf = C.create_string_buffer(max(1, n.value))
        self._ck(self.lib.bzk_params_read(self.h, ph, which, buf, n.value, None), "params_read")
        return buf.raw[: n.value]

    def groth16_setup(self, csr_abc, n_in: int, n_aux: int, toxic: bytes):
        """csr_abc: three (n_rows, row_ptr_bytes(u32), col_bytes(u32), val_bytes) tuples.  Returns (params handle,
        vk bincode bytes = Groth16VerifyingKey)."""
        keep, descs = [], []
        for n_rows, rp, col, val in csr_abc:
            # bytes are copied into stable buffers; ctypes arrays (R1cs.raw: zero-copy views of the generator's own
            # arrays - the only option once a matrix passes 2 GiB) are passed by address
            bufs = [x if isinstance(x, C.Array) else C.create_string_buffer(bytes(x), max(1, len(x))) for x in (rp, col, val)]
            keep.append(bufs)
            descs.append(CsrDesc(n_rows, *[C.cast(C.addressof(b), C.c_void_p) for b in bufs]))
        h = C.c_void_p()
        vk = C.create_string_buffer(878 + 97 * n_in)
        self._ck(self.lib.bzk_groth16_setup(self.h, C.byref(descs[0]), C.byref(descs[1]), C.byref(descs[2]), n_in, n_aux,
                                            _ptr(toxic), C.byref(h), vk, len(vk)), "groth16_setup")
        return h, vk.raw

    # ---- the phase-2 step of a ceremony: delta times d (include/bzk.h)
    def g1_scale_batch(self, pts: bytes, k: bytes):
        """(out, inf): k times each raw 96-byte G1 point, one lane per point; k one Montgomery Fr scalar"""
        return g1_scale_batch(self, pts, k)

    def g1_scale_batch_dev(self, pts, n: int, k: bytes, out, inf=None):
        """device buffers: pts and out n x 96 (out may be pts), inf n flag bytes or None; synchronises"""
        self._ck(self.lib.bzk_g1_scale_batch_dev(self.h, _ptr(pts), n, _ptr(k), _ptr(out), _ptr(inf) if inf is not None else None),
                 "g1_scale_batch_dev")

    def params_rekey(self, ph, d: bytes):
        """(new params handle, its 870-byte vk head): the resident key `ph` with delta times d; `ph` is left as it was"""
        return params_rekey(self, ph, d)

    def bellman_params_rekey(self, blob: bytes, d: bytes) -> bytes:
        return bellman_params_rekey(self, blob, d)

    def bellman_params_rekey_check(self, before: bytes, after: bytes, seed: bytes):
        return bellman_params_rekey_check(self, before, after, seed)

    # ---- n points times n scalars, the powers form and the powers-of-tau accumulator (include/bzk.h)
    def mul_batch(self, group: str, pts: bytes, scalars: bytes, canonical: bool = False):
        """(out, inf): scalars[i] times each raw G1 / G2 point, one lane per point"""
        return mul_batch(self, group, pts, scalars, canonical)

    def mul_batch_dev(self, group: str, pts, scalars, n: int, out, inf=None, canonical: bool = False):
        """device buffers: pts and out n records (out may be pts), scalars n x 32, inf n flag bytes or None; synchronises"""
        fn = {"g1": self.lib.bzk_g1_mul_batch_dev, "g2": self.lib.bzk_g2_mul_batch_dev}[group]
        self._ck(fn(self.h, _ptr(pts), _ptr(scalars), n, BZK_F_CANONICAL if canonical else 0, _ptr(out), _ptr(inf) if inf is not None else None),
                 "mul_batch_dev")

    def mul_powers(self, group: str, pts: bytes, c: bytes, s: bytes, start: int = 0):
        """(out, inf): c s^(start + i) times point i; c, s Montgomery Fr scalars"""
        return mul_powers(self, group, pts, c, s, start)

    def mul_powers_dev(self, group: str, pts, n: int, c: bytes, s: bytes, start: int, out, inf=None):
        fn = {"g1": self.lib.bzk_g1_mul_powers_dev, "g2": self.lib.bzk_g2_mul_powers_dev}[group]
        self._ck(fn(self.h, _ptr(pts), n, _ptr(c), _ptr(s), start, _ptr(out), _ptr(inf) if inf is not None else None), "mul_powers_dev")

    def ptau_contribute(self, blob: bytes, secrets: bytes):
        """(new accumulator, 576-byte key): the five arrays' powers calls on the device"""
        return ptau_contribute(self, blob, secrets)

    def ptau_check(self, before, key, after: bytes, seed: bytes):
        return ptau_check(self, before, key, after, seed)

    def groth16_h_dev(self, a, b, c, log_m: int):
        self._ck(self.lib.bzk_groth16_h_dev(self.h, _ptr(a), _ptr(b), _ptr(c), log_m), "groth16_h_dev")

    def g1_synth_bases_dev(self, seed: int, start: int, n: int, out):
        # test / bench helper: synchronised, so that a caller reading `out` through another stream (torch) cannot race the kernel
        self._ck(self.lib.bzk_g1_synth_bases_dev(self.h, seed, start, n, _ptr(out)), "g1_synth_bases_dev")
        self.sync()

    def g2_synth_bases_dev(self, seed: int, start: int, n: int, out):
        self._ck(self.lib.bzk_g2_synth_bases_dev(self.h, seed, start, n, _ptr(out)), "g2_synth_bases_dev")
        self.sync()


# --------------------------------------------------------------------------------------------------
# host-side (CPU, C++) MPN witness / R1CS generator - no GPU needed
# --------------------------------------------------------------------------------------------------
MG_X_AUTO, MG_X_HOST, MG_X_PEER, MG_X_RCCL = 0, 1, 2, 3
MG_X_NAMES = {MG_X_HOST: "host", MG_X_PEER: "peer", MG_X_RCCL: "rccl"}


def mg_probe(device: int) -> int:
    """bit 0: the device is a usable gfx950; bit 1: librccl loads with everything the RCCL exchange needs (bzk_mg_probe)"""
    st = load_library().bzk_mg_probe(device)
    if st < 0:
        raise BzkError(f"bzk_mg_probe: {load_library().bzk_strerror(st).decode()}")
    return st


def mg_unique_id() -> bytes:
    """group id of a process-per-GPU deployment: rank 0 draws it, the host hands it to the other ranks (bzk_mg_unique_id)"""
    lib = load_library()
    out = C.create_string_buffer(128)
    st = lib.bzk_mg_unique_id(out)
    if st != 0:
        raise BzkError(f"bzk_mg_unique_id: {lib.bzk_strerror(st).decode()}")
    return out.raw


class Mg:
    """A device group behind the C ABI (include/bzk.h row (e)): window-sharded MSMs and a proof pool over 1..8 GPUs.
    Mg(devices=[0, 1, ...])                 one process drives the devices
    Mg(device=d, rank=r, world=N, uid=...)  one process per GPU (uid from mg_unique_id() on rank 0)"""

    def __init__(self, devices=None, device=None, rank=None, world=None, uid=None, exchange=MG_X_AUTO):
        self.lib = load_library()
        h = C.c_void_p()
        if devices is not None:
            arr = (_i32 * len(devices))(*devices)
            st = self.lib.bzk_mg_create(arr, len(devices), exchange, C.byref(h))
        else:
            st = self.lib.bzk_mg_create_rank(device, rank, world, _ptr(uid), exchange, C.byref(h))
        if st != 0:
            raise BzkError(f"bzk_mg_create: {self.lib.bzk_strerror(st).decode()}")
        self.h = h
        self.world, self.local, self.rank = self.lib.bzk_mg_world(h), self.lib.bzk_mg_local(h), self.lib.bzk_mg_rank(h)
        self.exchange = MG_X_NAMES.get(self.lib.bzk_mg_exchange(h), "?")

    def close(self):
        if getattr(self, "h", None):
            self.lib.bzk_mg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st, what):
        if st != 0:
            raise BzkError(f"{what}: {self.lib.bzk_strerror(st).decode()} [{self.lib.bzk_mg_last_error(self.h).decode()}]")

    def _ptrs(self, xs):
        assert len(xs) == self.local, "one device pointer per local device"
        return (_vp * self.local)(*[_ptr(x) for x in xs])

    def stats(self, reset: bool = False) -> dict:
        """where this rank's window-sharded calls spent their time (bzk_mg_stats)"""
        v = (C.c_double * 8)()
        self._ck(self.lib.bzk_mg_stats(self.h, int(reset), v), "mg_stats")
        return {"calls": int(v[0]), "local_ms": v[1], "exchange_ms": v[2], "peer_wait_ms": v[3], "combine_ms": v[4], "create_s": v[5],
                "comm_init_s": v[6]}

    def ctx_handle(self, i: int):
        return self.lib.bzk_mg_ctx(self.h, i)

    def bases_load(self, bases_host: bytes, n: int, g2=False):
        h = C.c_void_p()
        fn = self.lib.bzk_mg_bases_g2_load if g2 else self.lib.bzk_mg_bases_g1_load
        self._ck(fn(self.h, _ptr(bases_host), n, C.byref(h)), "mg_bases_load")
        return h

    def bases_load_dev(self, bases_dev, n: int, g2=False):
        h = C.c_void_p()
        fn = self.lib.bzk_mg_bases_g2_load_dev if g2 else self.lib.bzk_mg_bases_g1_load_dev
        self._ck(fn(self.h, self._ptrs(bases_dev), n, C.byref(h)), "mg_bases_load_dev")
        return h

    def bases_free(self, handle):
        self.lib.bzk_mg_bases_free(self.h, handle)

    def msm(self, bases, scalars_host: bytes, n: int, g2=False, canonical=False, dedup=False, throughput=False) -> bytes:
        out = C.create_string_buffer(193 if g2 else 97)
        fn = self.lib.bzk_mg_msm_g2 if g2 else self.lib.bzk_mg_msm_g1
        self._ck(fn(self.h, bases, _ptr(scalars_host), n, _flags(canonical, dedup, throughput), out), "mg_msm")
        return out.raw

    def msm_dev(self, bases, scalars_dev, n: int, g2=False, canonical=False, dedup=False, throughput=False) -> bytes:
        out = C.create_string_buffer(193 if g2 else 97)
        fn = self.lib.bzk_mg_msm_g2_dev if g2 else self.lib.bzk_mg_msm_g1_dev
        self._ck(fn(self.h, bases, self._ptrs(scalars_dev), n, _flags(canonical, dedup, throughput), out), "mg_msm_dev")
        return out.raw

    # ---- proof pool
    def params_load(self, params: dict, slots_per_device: int = 2):
        keep = {k: C.create_string_buffer(bytes(params[k]), max(1, len(params[k])))
                for k in ("vk", "h", "l", "a", "b_g1", "b_g2", "a_density", "b_density")}
        d = ParamsDesc(params["n_in"], params["n_aux"], params["log_m"], params["n_a"], params["n_b"],
                       *[C.cast(keep[k], C.c_void_p) for k in ("vk", "h", "l", "a", "b_g1", "b_g2", "a_density", "b_density")])
        h = C.c_void_p()
        self._ck(self.lib.bzk_mg_params_load(self.h, C.byref(d), slots_per_device, C.byref(h)), "mg_params_load")
        return h

    def params_free(self, ph):
        self.lib.bzk_mg_params_free(self.h, ph)

    def params_stats(self, ph):
        n = self.lib.bzk_mg_params_slots(ph)
        arr = (_u64 * max(1, n))()
        self._ck(self.lib.bzk_mg_params_stats(ph, arr, n), "mg_params_stats")
        return list(arr)[:n]

    def prove_submit(self, ph, z, az, bz, cz, r: bytes, s: bytes):
        """returns a pending-proof record; keep it (it owns the buffers) until prove_wait"""
        asg = Assignment(*[_ptr(x) for x in (z, az, bz, cz)], len(az) // 32, len(z) // 32)
        out = C.create_string_buffer(387)
        t = _u64()
        self._ck(self.lib.bzk_mg_prove_submit(self.h, ph, C.byref(asg), _ptr(r), _ptr(s), out, C.byref(t)), "mg_prove_submit")
        return {"ticket": t.value, "out": out, "keep": (asg, z, az, bz, cz, r, s), "ph": ph}

    def prove_wait(self, pending) -> bytes:
        self._ck(self.lib.bzk_mg_prove_wait(self.h, pending["ph"], pending["ticket"]), "mg_prove_wait")
        return pending["out"].raw


def _st(st, what):
    if st != 0:
        raise BzkError(f"{what}: {load_library().bzk_strerror(st).decode()}")


def _ck_ctx(ctx_h, st, what):
    """raises with bzk_last_error of the context - of this thread's ctx = NULL route when there is none"""
    if st != 0:
        lib = load_library()
        raise BzkError(f"{what}: {lib.bzk_strerror(st).decode()} [{lib.bzk_last_error(ctx_h).decode()}]", st)


def _r1cs_mats_load(ctx_h, csr_abc, n_in, n_aux):
    lib = load_library()
    keep, descs = [], []
    for n_rows, rp, col, val in csr_abc:
        # None stays a NULL pointer (the loader refuses it unless the count is zero); bytes are copied, ctypes arrays passed by address
        bufs = [x if x is None or isinstance(x, C.Array) else C.create_string_buffer(bytes(x), max(1, len(x))) for x in (rp, col, val)]
        keep.append(bufs)
        descs.append(CsrDesc(n_rows, *[None if b is None else C.cast(C.addressof(b), C.c_void_p) for b in bufs]))
    h = C.c_void_p()
    _ck_ctx(ctx_h, lib.bzk_r1cs_mats_load(ctx_h, C.byref(descs[0]), C.byref(descs[1]), C.byref(descs[2]), n_in, n_aux, C.byref(h)), "r1cs_mats_load")
    return h


def _r1cs_mats_from(ctx_h, r1cs):
    h = C.c_void_p()
    _ck_ctx(ctx_h, load_library().bzk_r1cs_mats_from_r1cs(ctx_h, r1cs.h, C.byref(h)), "r1cs_mats_from_r1cs")
    return h


def _r1cs_eval(ctx_h, mh, z, want_unsat):
    lib = load_library()
    n_rows = r1cs_mats_info(mh)["n_rows"]
    zz = bytes(z) if isinstance(z, bytearray) else z
    outs = [C.create_string_buffer(max(1, 32 * n_rows)) for _ in range(3)]
    first = C.c_int64(-2)
    _ck_ctx(ctx_h, lib.bzk_r1cs_eval(ctx_h, mh, _ptr(zz), len(zz) // 32, outs[0], outs[1], outs[2], C.byref(first) if want_unsat else None), "r1cs_eval")
    res = tuple(o.raw[: 32 * n_rows] for o in outs)
    return res + (first.value,) if want_unsat else res


def r1cs_mats_load(csr_abc, n_in: int, n_aux: int):
    """ctx = NULL: the matrices kept in host memory, for r1cs_eval below (host threads).  csr_abc as Bzk.groth16_setup takes it."""
    return _r1cs_mats_load(None, csr_abc, n_in, n_aux)


def r1cs_mats_from(r1cs):
    return _r1cs_mats_from(None, r1cs)


def r1cs_mats_free(mh):
    load_library().bzk_r1cs_mats_free(None, mh)


def r1cs_mats_info(mh) -> dict:
    info = (_u64 * 8)()
    _st(load_library().bzk_r1cs_mats_info(mh, info), "r1cs_mats_info")
    return dict(zip(("n_rows", "n_vars", "nnzA", "nnzB", "nnzC", "n_coeffs", "resident_bytes"), [int(x) for x in info]))


def r1cs_eval(mh, z, want_unsat: bool = False):
    """(az, bz, cz[, first unsatisfied row or -1]) on host threads, from a handle loaded without a context"""
    return _r1cs_eval(None, mh, z, want_unsat)


class R1cs:
    """A synthesized circuit instance (assignment + optional CSR matrices)."""
    VIEWS = {"z": 0, "az": 1, "bz": 2, "cz": 3, "a_density": 4, "b_density": 5, "valA": 6, "valB": 7, "valC": 8,
             "colA": 9, "colB": 10, "colC": 11, "rpA": 12, "rpB": 13, "rpC": 14}

    def __init__(self, handle):
        self.lib = load_library()
        self.h = handle
        info = (_u64 * 9)()
        _st(self.lib.bzk_r1cs_info(self.h, info), "r1cs_info")
        (self.n_in, self.n_aux, self.n_constraints, self.nnzA, self.nnzB, self.nnzC, first_bad, self.accepted,
         self.rejected) = [int(x) for x in info]
        self.first_unsatisfied = first_bad - 1
        self.satisfied = first_bad == 0

    DEFER_FIELDS = ("deferred", "n_tx", "n_ops", "n_regs", "n_inputs", "n_levels", "hole_aux", "hole_con", "filled", "flags")

    def defer_info(self) -> dict:
        """what a synthesis with MpnWorld.set_defer(True) left to the device (bzk_r1cs_defer_info)"""
        info = (_u64 * 10)()
        _st(self.lib.bzk_r1cs_defer_info(self.h, info), "r1cs_defer_info")
        return dict(zip(self.DEFER_FIELDS, [int(x) for x in info]))

    def defer_schedule_info(self) -> dict:
        """the one-launch device schedule of this instance's deferred-value program, checked on the host (bzk_r1cs_defer_schedule_info)"""
        info = (_u64 * 6)()
        _st(self.lib.bzk_r1cs_defer_schedule_info(self.h, info), "r1cs_defer_schedule_info")
        return dict(zip(("stages", "segments", "hash_ops", "fill_ops", "largest_segment", "violations"), [int(x) for x in info]))

    def fill_host(self) -> dict:
        """runs the instance's deferred-value program on the CPU (same ops as the device): the views are complete afterwards"""
        _st(self.lib.bzk_r1cs_fill_host(self.h), "r1cs_fill_host")
        return self.defer_info()

    def view(self, name: str) -> bytes:
        """a COPY of the array as bytes (tests); the prover path uses raw()"""
        n = _u64()
        p = self.lib.bzk_r1cs_data(self.h, self.VIEWS[name], C.byref(n))
        return C.string_at(p, n.value) if n.value else b""

    def raw(self, name: str):
        """zero-copy ctypes view of the array inside the generator's (pinned) buffer; valid while this object lives"""
        n = _u64()
        p = self.lib.bzk_r1cs_data(self.h, self.VIEWS[name], C.byref(n))
        arr = (C.c_char * max(1, n.value)).from_address(p) if n.value else (C.c_char * 1)()
        arr._owner = self
        return arr

    def free(self):
        if self.h:
            self.lib.bzk_r1cs_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MpnWorld:
    def __init__(self, log4_tree: int, log4_token_tree: int):
        self.lib = load_library()
        h = C.c_void_p()
        _st(self.lib.bzk_mpn_create(log4_tree, log4_token_tree, C.byref(h)), "mpn_create")
        self.h = h

    def close(self):
        if self.h:
            self.lib.bzk_mpn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_height(self, height: int):
        _st(self.lib.bzk_mpn_set_height(self.h, height), "set_height")

    def set_threads(self, n: int):
        _st(self.lib.bzk_mpn_set_threads(self.h, n), "set_threads")

    def set_defer(self, on: bool = True):
        """witness-only update instances leave the hash-dependent values to the device (Bzk.groth16_prove_r1cs) or to R1cs.fill_host"""
        _st(self.lib.bzk_mpn_set_defer(self.h, 1 if on else 0), "set_defer")

    def set_defer_sig(self, on: bool = True):
        """set_defer and, beyond it, the EdDSA gadget's ladders (bzk_mpn_set_defer_sig); off: back to plain deferral"""
        _st(self.lib.bzk_mpn_set_defer_sig(self.h, 1 if on else 0), "set_defer_sig")

    def set_device(self, ctx):
        """ctx: a Bzk context (kept alive by this object) whose GPU batches the builders' Merkle hashing; None: host path"""
        self._dev = ctx
        _st(self.lib.bzk_mpn_set_device(self.h, ctx.h if ctx is not None else None), "set_device")

    def add_account(self, index: int, seed: bytes, token_id: bytes, balance: int) -> bytes:
        out = C.create_string_buffer(64)
        _st(self.lib.bzk_mpn_add_account(self.h, index, _ptr(seed), len(seed), _ptr(token_id), balance, out), "add_account")
        return out.raw

    def add_key(self, index: int, seed: bytes):
        _st(self.lib.bzk_mpn_add_key(self.h, index, _ptr(seed), len(seed)), "add_key")

    def root(self) -> bytes:
        out = C.create_string_buffer(32)
        _st(self.lib.bzk_mpn_root(self.h, out), "root")
        return out.raw

    def push_tx(self, src: int, dst: int, token_id: bytes, amount: int, fee_token: bytes, fee: int):
        _st(self.lib.bzk_mpn_push_tx(self.h, src, dst, _ptr(token_id), amount, _ptr(fee_token), fee), "push_tx")

    def push_txs(self, txs: bytes, n: int):
        """mempool admission of n wire-form transactions (consecutive bincode(MpnTransaction)): (verdict bytes, number queued).  Checked on the
        device when set_device was given a context, else on host threads; those that verify are queued in input order"""
        ok, acc = C.create_string_buffer(max(n, 1)), _u64()
        st = self.lib.bzk_mpn_push_txs(self.h, _ptr(txs), len(txs), n, ok, C.byref(acc))
        if st != 0:
            raise BzkError(f"push_txs: {self.lib.bzk_strerror(st).decode()} [{self.lib.bzk_mpn_work_last_error().decode()}]")
        return ok.raw[:n], acc.value

    def push_withdraws(self, txs: bytes, n: int):
        """mempool admission of n wire-form withdrawals (consecutive bincode(MpnWithdraw)): (1 / 0 per record, number queued).  Checked on the
        device when set_device was given a context, else on host threads; the accepted ones are queued in input order with their payments"""
        ok, acc = C.create_string_buffer(max(n, 1)), _u64()
        st = self.lib.bzk_mpn_push_withdraws(self.h, _ptr(txs), len(txs), n, ok, C.byref(acc))
        if st != 0:
            raise BzkError(f"push_withdraws: {self.lib.bzk_strerror(st).decode()} [{self.lib.bzk_mpn_work_last_error().decode()}]")
        return ok.raw[:n], acc.value

    def push_deposits(self, txs: bytes, n: int):
        """mempool admission of n wire-form deposits (consecutive bincode(MpnDeposit)): (1 / 0 per record, number queued).  Checked on the
        device when set_device was given a context, else on host threads; the accepted ones are queued in input order with their payments"""
        ok, acc = C.create_string_buffer(max(n, 1)), _u64()
        st = self.lib.bzk_mpn_push_deposits(self.h, _ptr(txs), len(txs), n, ok, C.byref(acc))
        if st != 0:
            raise BzkError(f"push_deposits: {self.lib.bzk_strerror(st).decode()} [{self.lib.bzk_mpn_work_last_error().decode()}]")
        return ok.raw[:n], acc.value

    def push_deposit(self, key_index: int, token_id: bytes, amount: int):
        _st(self.lib.bzk_mpn_push_deposit(self.h, key_index, _ptr(token_id), amount), "push_deposit")

    def push_withdraw(self, account: int, token_id: bytes, amount: int, fee_token: bytes, fee: int, fingerprint: bytes | None = None):
        """fingerprint None: derived from a synthetic L1 payment as the wallet does (the withdrawal can go on the wire)"""
        _st(self.lib.bzk_mpn_push_withdraw(self.h, account, _ptr(token_id), amount, _ptr(fee_token), fee, _ptr(fingerprint)), "push_withdraw")

    def push_withdraw_signed(self, pub_xy: bytes, nonce: int, token_id: bytes, amount: int, fee_token: bytes, fee: int, fingerprint: bytes, sig: bytes):
        """a withdrawal signed elsewhere (sig = r.x | r.y | s over H2(fingerprint, nonce)), queued as given; the builder checks it"""
        _st(self.lib.bzk_mpn_push_withdraw_signed(self.h, _ptr(pub_xy), nonce, _ptr(token_id), amount, _ptr(fee_token), fee, _ptr(fingerprint),
                                                  _ptr(sig)), "push_withdraw_signed")

    def make_work(self, kind: int, vks, reward: int, log4_batches=(1, 1, 1), num_batches=(1, 1, 1), state_size: int = 0) -> "MpnWork":
        """validator side (`prepare_works`): one work from the queued transactions.  kind 0 deposit / 1 withdraw / 2 update;
        vks = (deposit, withdraw, update) bincode Groth16VerifyingKey; log4_batches = (deposit, withdraw, update);
        num_batches = (update, deposit, withdraw) counts of MpnConfig."""
        keep = [C.create_string_buffer(bytes(v), len(v)) for v in vks]
        cfg = WorkConfig(log4_batches[0], log4_batches[1], log4_batches[2], num_batches[0], num_batches[1], num_batches[2],
                         C.cast(keep[0], _vp), len(vks[0]), C.cast(keep[1], _vp), len(vks[1]), C.cast(keep[2], _vp), len(vks[2]),
                         state_size)
        h = C.c_void_p()
        _st(self.lib.bzk_mpn_make_work(self.h, kind, C.byref(cfg), reward, C.byref(h)), "make_work")
        return MpnWork(h)

    def deposit_synthesize(self, log4_batch: int, commitment: bytes, record_matrices=False) -> R1cs:
        h = C.c_void_p()
        _st(self.lib.bzk_mpn_deposit_synthesize(self.h, log4_batch, _ptr(commitment), int(record_matrices), C.byref(h)), "deposit_synthesize")
        return R1cs(h)

    def withdraw_synthesize(self, log4_batch: int, commitment: bytes, record_matrices=False) -> R1cs:
        h = C.c_void_p()
        _st(self.lib.bzk_mpn_withdraw_synthesize(self.h, log4_batch, _ptr(commitment), int(record_matrices), C.byref(h)), "withdraw_synthesize")
        return R1cs(h)

    def update_synthesize(self, log4_batch: int, commitment: bytes, fee_token: bytes, record_matrices=False) -> R1cs:
        h = C.c_void_p()
        _st(self.lib.bzk_mpn_update_synthesize(self.h, log4_batch, _ptr(commitment), _ptr(fee_token), int(record_matrices),
                                               C.byref(h)), "update_synthesize")
        return R1cs(h)


class MpnWork:
    """One `MpnWork` (src/mpn/mod.rs:263-270): decoded from bincode bytes (worker side) or made from a world (validator side)."""
    KINDS = ("deposit", "withdraw", "update")

    def __init__(self, handle, consumed: int = 0):
        self.lib = load_library()
        self.h = handle
        self.consumed = consumed
        info = (_u64 * 12)()
        _st(self.lib.bzk_mpn_work_info(self.h, info), "work_info")
        (self.kind, self.log4_tree, self.log4_token_tree, self.log4_batch, self.n_transitions, self.height, self.reward,
         self.new_root_size, self.num_update_batches, self.num_deposit_batches, self.num_withdraw_batches, self.vk_len) = [int(x) for x in info]
        sc = C.create_string_buffer(160)
        _st(self.lib.bzk_mpn_work_scalars(self.h, sc), "work_scalars")
        self.state, self.aux_data, self.next_state, self.new_root_hash, self.contract_id = [sc.raw[32 * i:32 * i + 32] for i in range(5)]

    @classmethod
    def decode(cls, data, flags: int = 0, offset: int = 0) -> "MpnWork":
        """decodes the work at data[offset:] (bytes or a ctypes buffer) without slicing - a response holds several works"""
        lib = load_library()
        h, used = C.c_void_p(), _u64()
        if offset < 0 or offset > len(data):
            raise BzkError("work_decode: offset out of range")
        base = _ptr(data)
        at = C.c_void_p((base.value or 0) + offset) if offset else base
        st = lib.bzk_mpn_work_decode(at, len(data) - offset, flags, C.byref(h), C.byref(used))
        if st != 0:
            raise BzkError(f"work_decode: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
        return cls(h, used.value)

    def free(self):
        if self.h:
            self.lib.bzk_mpn_work_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def vk(self, which: int = -1) -> bytes:
        n = _u64()
        _st(self.lib.bzk_mpn_work_vk(self.h, which, None, 0, C.byref(n)), "work_vk")
        buf = C.create_string_buffer(max(1, n.value))
        _st(self.lib.bzk_mpn_work_vk(self.h, which, buf, n.value, None), "work_vk")
        return buf.raw[: n.value]

    def commitment(self, prover_pub: bytes) -> bytes:
        out = C.create_string_buffer(32)
        _st(self.lib.bzk_mpn_work_commitment(self.h, _ptr(prover_pub), out), "work_commitment")
        return out.raw

    def verify(self, prover_pub: bytes, proof387: bytes) -> bool:
        """`MpnWork::verify` (src/mpn/mod.rs:281-295), on the host"""
        st = self.lib.bzk_mpn_work_verify(self.h, _ptr(prover_pub), _ptr(proof387))
        if st < 0:
            raise BzkError(f"work_verify: {self.lib.bzk_strerror(st).decode()}")
        return st == 1

    def encode(self) -> bytes:
        n = _u64()
        _st(self.lib.bzk_mpn_work_encode(self.h, None, 0, C.byref(n)), "work_encode")
        buf = C.create_string_buffer(max(1, n.value))
        _st(self.lib.bzk_mpn_work_encode(self.h, buf, n.value, None), "work_encode")
        return buf.raw[: n.value]

    def synthesize(self, prover_pub: bytes, fee_token: bytes | None = None, threads: int = 0, record_matrices=False, defer=False) -> R1cs:
        """defer: BZK_SYNTH_DEFER - a work's hash-dependent values (all three kinds: update, deposit, withdraw) are left to the device (Bzk.groth16_prove_r1cs) / R1cs.fill_host;
        defer="sig": BZK_SYNTH_DEFER_SIG - the same, and the EdDSA gadget of every update / withdraw transition as well"""
        if defer == "sig":
            mode = BZK_SYNTH_DEFER_SIG
        elif isinstance(defer, str):
            raise ValueError(f"defer={defer!r}: True, False or 'sig'")
        else:
            mode = BZK_SYNTH_DEFER if defer else int(record_matrices)
        h = C.c_void_p()
        _st(self.lib.bzk_mpn_work_synthesize(self.h, _ptr(prover_pub), _ptr(fee_token), threads, mode, C.byref(h)), "work_synthesize")
        return R1cs(h)


def bellman_params_decode(blob: bytes, threads: int = 0) -> dict:
    """bellman `Parameters::write` bytes -> dict(vk (870 packed), ic (97 B each), h, l, a, b_g1 (raw 96 B), b_g2 (raw 192 B), counts)"""
    lib = load_library()
    info = (_u64 * 7)()
    _st(lib.bzk_bellman_params_info(_ptr(blob), len(blob), info), "bellman_params_info")
    n_ic, n_h, n_l, n_a, n_b1, n_b2, used = [int(x) for x in info]
    bufs = {k: C.create_string_buffer(max(1, sz)) for k, sz in dict(vk=870, ic=97 * n_ic, h=96 * n_h, l=96 * n_l, a=96 * n_a, b_g1=96 * n_b1,
                                                                     b_g2=192 * n_b2).items()}
    _st(lib.bzk_bellman_params_decode(_ptr(blob), len(blob), bufs["vk"], bufs["ic"], bufs["h"], bufs["l"], bufs["a"], bufs["b_g1"],
                                      bufs["b_g2"], threads), "bellman_params_decode")
    sizes = dict(vk=870, ic=97 * n_ic, h=96 * n_h, l=96 * n_l, a=96 * n_a, b_g1=96 * n_b1, b_g2=192 * n_b2)
    out = {k: v.raw[: sizes[k]] for k, v in bufs.items()}
    out.update(n_ic=n_ic, n_h=n_h, n_l=n_l, n_a=n_a, n_b_g1=n_b1, n_b_g2=n_b2, consumed=used)
    return out


def bellman_params_encode(vk870: bytes, ic: bytes, h: bytes, l: bytes, a: bytes, b_g1: bytes, b_g2: bytes) -> bytes:
    lib = load_library()
    n = _u64()
    args = (_ptr(vk870), _ptr(ic), len(ic) // 97, _ptr(h), len(h) // 96, _ptr(l), len(l) // 96, _ptr(a), len(a) // 96, _ptr(b_g1), _ptr(b_g2),
            len(b_g1) // 96)
    _st(lib.bzk_bellman_params_encode(*args, None, 0, C.byref(n)), "bellman_params_encode")
    buf = C.create_string_buffer(n.value)
    _st(lib.bzk_bellman_params_encode(*args, buf, n.value, None), "bellman_params_encode")
    return buf.raw


def host_default_threads() -> int:
    """the host generator's default thread count (visible CPUs capped by the cgroup CPU quota; BZK_HOST_THREADS overrides)"""
    return int(load_library().bzk_host_default_threads())


def groth16_verify(vk_bincode: bytes, inputs: bytes, proof387: bytes) -> bool:
    """host-side `groth16_verify` (src/zk/groth16/mod.rs:67-121): inputs = n x 32 B Montgomery scalars"""
    st = load_library().bzk_groth16_verify(_ptr(vk_bincode), len(vk_bincode), _ptr(inputs), len(inputs) // 32, _ptr(proof387))
    if st < 0:
        raise BzkError(f"groth16_verify: {load_library().bzk_strerror(st).decode()}")
    return st == 1


def zkproof_encode(proof387: bytes) -> bytes:
    out = C.create_string_buffer(391)
    _st(load_library().bzk_zkproof_encode(_ptr(proof387), out), "zkproof_encode")
    return out.raw


def zkproof_decode(data: bytes) -> bytes:
    out = C.create_string_buffer(387)
    _st(load_library().bzk_zkproof_decode(_ptr(data), len(data), out), "zkproof_decode")
    return out.raw


def mpn_update_empty(L, T, B, commitment, height, state, aux, next_state, fee_token, record_matrices=False) -> R1cs:
    h = C.c_void_p()
    _st(load_library().bzk_mpn_update_empty(L, T, B, _ptr(commitment), height, _ptr(state), _ptr(aux), _ptr(next_state),
                                            _ptr(fee_token), int(record_matrices), C.byref(h)), "update_empty")
    return R1cs(h)


def mpn_circuit_empty(kind, L, T, B, commitment, height, state, aux, next_state, record_matrices=False) -> R1cs:
    """kind: 0 deposit, 1 withdraw"""
    h = C.c_void_p()
    _st(load_library().bzk_mpn_circuit_empty(kind, L, T, B, _ptr(commitment), height, _ptr(state), _ptr(aux), _ptr(next_state),
                                             int(record_matrices), C.byref(h)), "circuit_empty")
    return R1cs(h)


def _csr(locators):
    off, loc = [0], []
    for l in locators:
        loc.extend(int(x) for x in l)
        off.append(len(loc))
    return (_u64 * len(off))(*off), (_u64 * max(1, len(loc)))(*loc)


CHAIN_APPLIED, CHAIN_MISMATCH, CHAIN_REFUSED, CHAIN_NOT_REACHED = 0, 1, 2, 3  # BZK_CHAIN_*


class DeviceState:
    """`KvStoreStateManager` for one contract with the values resident on the device (bzk_state_*): update / root / get / prove"""

    def __init__(self, ctx: "Bzk", model_bincode: bytes):
        self.ctx, self.lib, self.h = ctx, ctx.lib, _vp()
        ctx._ck(self.lib.bzk_state_create(ctx.h, _ptr(model_bincode), len(model_bincode), C.byref(self.h)), "state_create")

    def close(self):
        if self.h:
            self.lib.bzk_state_free(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            import sys
            if not sys.is_finalizing():    # at interpreter exit the HIP runtime may be gone already; the process frees the memory
                self.close()
        except Exception:
            pass

    def update(self, pairs, target_height: int, want_rollback=False):
        """pairs: iterable of (locator, 32-byte Montgomery scalar; zero = remove) -> (state_hash, state_size[, previous values])"""
        pairs = list(pairs)
        o, lo = _csr(l for l, _ in pairs)
        vals = b"".join(v for _, v in pairs)
        out, size = C.create_string_buffer(32), _u64()
        prev = C.create_string_buffer(max(1, 32 * len(pairs))) if want_rollback else None
        self.ctx._ck(self.lib.bzk_state_update(self.h, o, lo, _ptr(vals), len(pairs), target_height, out, C.byref(size), prev), "state_update")
        if want_rollback:
            return out.raw, size.value, [prev.raw[32 * i:32 * i + 32] for i in range(len(pairs))]
        return out.raw, size.value

    def update_bincode(self, delta_bincode: bytes, target_height: int) -> bytes:
        out = C.create_string_buffer(40)
        self.ctx._ck(self.lib.bzk_state_update_bincode(self.h, _ptr(delta_bincode), len(delta_bincode), target_height, out), "state_update_bincode")
        return out.raw

    def update_chain(self, deltas, target_heights, claims=None, round_versions: int = 0, want_rollback=False):
        """deltas: m lists of (locator, 32-byte Montgomery scalar) as `update` takes them, applied in order while each is accepted and gives
        claims[j] (m x 40 bytes: state_hash | state_size; None: nothing can mismatch).  -> (applied, [CHAIN_* verdicts], [40-byte state per
        delta][, per delta the previous values of its pairs]).  A refused delta is a verdict: ctx.last_refusal() / last_error name it"""
        deltas = [list(d) for d in deltas]
        m, flat = len(deltas), [p for d in deltas for p in d]
        d_off = [0]
        for d in deltas:
            d_off.append(d_off[-1] + len(d))
        o, lo = _csr(l for l, _ in flat)
        vals = b"".join(v for _, v in flat)
        hs = (_u64 * max(1, m))(*[int(h) for h in target_heights])
        states, verdict, applied = C.create_string_buffer(max(1, 40 * m)), C.create_string_buffer(max(1, m)), _u64()
        prev = C.create_string_buffer(max(1, 32 * len(flat))) if want_rollback else None
        if claims is not None:
            claims = b"".join(claims) if not isinstance(claims, (bytes, bytearray)) else bytes(claims)
            assert len(claims) == 40 * m
        self.ctx._ck(self.lib.bzk_state_update_chain(self.h, m, (_u64 * len(d_off))(*d_off), o, lo, _ptr(vals) if vals else None, hs,
                                                     _ptr(claims) if claims else None, round_versions, states, verdict, C.byref(applied), prev),
                     "state_update_chain")
        out = (applied.value, list(verdict.raw[:m]), [states.raw[40 * j:40 * j + 40] for j in range(m)])
        if want_rollback:
            return out + ([[prev.raw[32 * i:32 * i + 32] for i in range(d_off[j], d_off[j + 1])] for j in range(m)],)
        return out

    def update_chain_bincode(self, blobs, target_heights, claims=None, round_versions: int = 0):
        """the same over m bincode(ZkDeltaPairs) blobs; one that does not decode is refused"""
        blobs = [bytes(b) for b in blobs]
        m = len(blobs)
        b_off = [0]
        for b in blobs:
            b_off.append(b_off[-1] + len(b))
        data = b"".join(blobs) or b"\0"
        hs = (_u64 * max(1, m))(*[int(h) for h in target_heights])
        states, verdict, applied = C.create_string_buffer(max(1, 40 * m)), C.create_string_buffer(max(1, m)), _u64()
        if claims is not None:
            claims = b"".join(claims) if not isinstance(claims, (bytes, bytearray)) else bytes(claims)
            assert len(claims) == 40 * m
        self.ctx._ck(self.lib.bzk_state_update_chain_bincode(self.h, m, _ptr(data), (_u64 * len(b_off))(*b_off), hs, _ptr(claims) if claims else None,
                                                             round_versions, states, verdict, C.byref(applied)), "state_update_chain_bincode")
        return applied.value, list(verdict.raw[:m]), [states.raw[40 * j:40 * j + 40] for j in range(m)]

    def root(self):
        """-> (state_hash, state_size, height)"""
        out, size, height = C.create_string_buffer(32), _u64(), _u64()
        self.ctx._ck(self.lib.bzk_state_root(self.h, out, C.byref(size), C.byref(height)), "state_root")
        return out.raw, size.value, height.value

    def get(self, locators) -> list:
        locators = list(locators)
        o, lo = _csr(locators)
        out = C.create_string_buffer(max(1, 32 * len(locators)))
        self.ctx._ck(self.lib.bzk_state_get(self.h, o, lo, len(locators), out), "state_get")
        return [out.raw[32 * i:32 * i + 32] for i in range(len(locators))]

    def prove(self, tree_loc, indices) -> list:
        """-> per index: log4_size levels (leaf level first) of three 32-byte siblings"""
        tree_loc, indices = [int(x) for x in tree_loc], [int(x) for x in indices]
        tl = (_u64 * max(1, len(tree_loc)))(*tree_loc)
        ix = (_u64 * max(1, len(indices)))(*indices)
        log4 = _u32()
        self.ctx._ck(self.lib.bzk_state_prove(self.h, tl, len(tree_loc), None, 0, None, C.byref(log4)), "state_prove")  # the depth
        out = C.create_string_buffer(max(1, len(indices) * log4.value * 96))
        self.ctx._ck(self.lib.bzk_state_prove(self.h, tl, len(tree_loc), ix, len(indices), out, C.byref(log4)), "state_prove")
        L, raw = log4.value, out.raw
        return [[[raw[((i * L + d) * 3 + j) * 32:((i * L + d) * 3 + j) * 32 + 32] for j in range(3)] for d in range(L)] for i in range(len(indices))]

    def stats(self) -> dict:
        a, b, c = _u64(), _u64(), _u64()
        self.ctx._ck(self.lib.bzk_state_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "state_stats")
        return {"slots": a.value, "device_bytes": b.value, "keys": c.value}


def state_model_default(model_bincode: bytes) -> bytes:
    """`ZkStateModel::compress_default` (host)"""
    out = C.create_string_buffer(32)
    _st(load_library().bzk_state_model_default(_ptr(model_bincode), len(model_bincode), out), "state_model_default")
    return out.raw


def host_poseidon(inp: bytes) -> bytes:
    out = C.create_string_buffer(32)
    _st(load_library().bzk_host_poseidon(_ptr(inp), len(inp) // 32, out), "host_poseidon")
    return out.raw


def host_scalar_new(le_bytes: bytes) -> bytes:
    """`ZkScalar::new`: little-endian integer mod r -> 32 Montgomery bytes"""
    out = C.create_string_buffer(32)
    _st(load_library().bzk_host_scalar_new(_ptr(le_bytes) if le_bytes else None, len(le_bytes), out), "host_scalar_new")
    return out.raw


def host_sha3_256(b: bytes) -> bytes:
    out = C.create_string_buffer(32)
    _st(load_library().bzk_host_sha3_256(_ptr(b) if b else None, len(b), out), "host_sha3")
    return out.raw


def host_jubjub_keys(seed: bytes) -> bytes:
    out = C.create_string_buffer(128)
    _st(load_library().bzk_host_jubjub_keys(_ptr(seed), len(seed), out), "jubjub_keys")
    return out.raw


def host_jubjub_sign(key: bytes, msg: bytes) -> bytes:
    out = C.create_string_buffer(96)
    _st(load_library().bzk_host_jubjub_sign(_ptr(key), _ptr(msg), out), "jubjub_sign")
    return out.raw


def host_jubjub_verify(pub_xy: bytes, msg: bytes, sig: bytes) -> bool:
    r = load_library().bzk_host_jubjub_verify(_ptr(pub_xy), _ptr(msg), _ptr(sig))
    if r < 0:
        raise BzkError("jubjub_verify: bad argument")
    return bool(r)


def host_jubjub_decompress(x: bytes, odd: bool):
    """PointCompressed::decompress on the host: x | y (64 bytes), or None where the reference panics or x is not a residue's limbs"""
    out = C.create_string_buffer(64)
    r = load_library().bzk_host_jubjub_decompress(_ptr(x), 1 if odd else 0, out)
    if r < 0:
        raise BzkError("jubjub_decompress: bad argument")
    return out.raw if r else None


JUBJUB_SIGN_ROUND = 1 << 16  # rows a host-pointer signing or key call stages per round (sign.hip SIGN_ROUND)
MPN_TX_CHUNK = 1 << 16  # wire-form records staged per round (bzk_mpn_wire.h MPN_TX_CHUNK)
MPN_WD_CHUNK_BYTES = 64 << 20  # payment bytes of wire-form withdrawals staged per round (bzk_mpn_wire.h MPN_WD_CHUNK_BYTES)


def _jubjub_keys_batch(ctx_handle, seeds) -> bytes:
    n = len(seeds)
    off = (_u64 * (n + 1))()
    for i, m in enumerate(seeds):
        off[i + 1] = off[i] + len(m)
    data = b"".join(seeds)
    out = C.create_string_buffer(max(128 * n, 1))
    _st(load_library().bzk_jubjub_keys_batch(ctx_handle, _ptr(data) if data else _ptr(b"\0"), off, n, out), "jubjub_keys_batch")
    return out.raw[: 128 * n]


def _jubjub_sign_batch(ctx_handle, keys: bytes, msg: bytes):
    n = len(msg) // 32
    if len(keys) != 128 * n or len(msg) != 32 * n:
        raise BzkError("jubjub_sign_batch: keys and msg describe different counts")
    sig, ok = C.create_string_buffer(max(96 * n, 1)), C.create_string_buffer(max(n, 1))
    _st(load_library().bzk_jubjub_sign_batch(ctx_handle, _ptr(keys), _ptr(msg), n, sig, ok), "jubjub_sign_batch")
    return sig.raw[: 96 * n], ok.raw[:n]


def _mpn_txs_sign(ctx_handle, keys: bytes, txs: bytes, n: int, want_hash: bool):
    lib = load_library()
    if len(keys) != 128 * n:
        raise BzkError("mpn_txs_sign: keys is not n x 128 bytes")
    out, ok = C.create_string_buffer(max(len(txs), 1)), C.create_string_buffer(max(n, 1))
    hashes = C.create_string_buffer(max(32 * n, 1)) if want_hash else None
    st = lib.bzk_mpn_txs_sign(ctx_handle, _ptr(keys), _ptr(txs), len(txs), n, out, ok, hashes)
    if st != 0:
        raise BzkError(f"mpn_txs_sign: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
    return out.raw[: len(txs)], ok.raw[:n], (hashes.raw[: 32 * n] if want_hash else None)


def _mpn_withdraws_sign(ctx_handle, keys: bytes, txs: bytes, n: int, want_fingerprint: bool):
    lib = load_library()
    if len(keys) != 128 * n:
        raise BzkError("mpn_withdraws_sign: keys is not n x 128 bytes")
    out, ok = C.create_string_buffer(max(len(txs), 1)), C.create_string_buffer(max(n, 1))
    fps = C.create_string_buffer(max(32 * n, 1)) if want_fingerprint else None
    st = lib.bzk_mpn_withdraws_sign(ctx_handle, _ptr(keys), _ptr(txs), len(txs), n, out, ok, fps)
    if st != 0:
        raise BzkError(f"mpn_withdraws_sign: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
    return out.raw[: len(txs)], ok.raw[:n], (fps.raw[: 32 * n] if want_fingerprint else None)


def host_jubjub_keys_batch(seeds) -> bytes:
    """Bzk.jubjub_keys_batch without a device: the same per-lane code on host threads"""
    return _jubjub_keys_batch(None, seeds)


def host_jubjub_sign_batch(keys: bytes, msg: bytes):
    """Bzk.jubjub_sign_batch without a device: the same per-lane code on host threads"""
    return _jubjub_sign_batch(None, keys, msg)


def host_mpn_txs_sign(keys: bytes, txs: bytes, n: int, want_hash: bool = True):
    """Bzk.mpn_txs_sign without a device: the same per-lane code on host threads"""
    return _mpn_txs_sign(None, keys, txs, n, want_hash)


def host_mpn_withdraws_sign(keys: bytes, txs: bytes, n: int, want_fingerprint: bool = True):
    """Bzk.mpn_withdraws_sign without a device: the same per-lane code on host threads"""
    return _mpn_withdraws_sign(None, keys, txs, n, want_fingerprint)


def _mpn_tx_verify_batch(ctx_handle, txs: bytes, n: int, want_hash: bool):
    lib = load_library()
    ok = C.create_string_buffer(max(n, 1))
    hashes = C.create_string_buffer(max(32 * n, 1)) if want_hash else None
    st = lib.bzk_mpn_tx_verify_batch(ctx_handle, _ptr(txs), len(txs), n, ok, hashes)
    if st != 0:
        raise BzkError(f"mpn_tx_verify_batch: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
    return ok.raw[:n], (hashes.raw[: 32 * n] if want_hash else None)


def host_mpn_tx_verify_batch(txs: bytes, n: int, want_hash: bool = True):
    """Bzk.mpn_tx_verify_batch without a device: the same verdicts and hashes on host threads"""
    return _mpn_tx_verify_batch(None, txs, n, want_hash)


def _mpn_withdraw_verify_batch(ctx_handle, txs: bytes, n: int, want_fingerprint: bool):
    lib = load_library()
    ok = C.create_string_buffer(max(n, 1))
    fps = C.create_string_buffer(max(32 * n, 1)) if want_fingerprint else None
    st = lib.bzk_mpn_withdraw_verify_batch(ctx_handle, _ptr(txs), len(txs), n, ok, fps)
    if st != 0:
        raise BzkError(f"mpn_withdraw_verify_batch: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
    return ok.raw[:n], (fps.raw[: 32 * n] if want_fingerprint else None)


def host_mpn_withdraw_verify_batch(txs: bytes, n: int, want_fingerprint: bool = True):
    """Bzk.mpn_withdraw_verify_batch without a device: the same verdicts and fingerprints on host threads"""
    return _mpn_withdraw_verify_batch(None, txs, n, want_fingerprint)


def _offsets(msgs):
    off = (_u64 * (len(msgs) + 1))()
    for i, m in enumerate(msgs):
        off[i + 1] = off[i] + len(m)
    return off, (b"".join(msgs) or b"\0")


def _sha512_batch(ctx_handle, msgs) -> bytes:
    n = len(msgs)
    off, data = _offsets(msgs)
    dig = C.create_string_buffer(max(64 * n, 1))
    _st(load_library().bzk_sha512_batch(ctx_handle, _ptr(data), off, n, dig), "sha512_batch")
    return dig.raw[: 64 * n]


def host_sha512_batch(msgs) -> bytes:
    """Bzk.sha512_batch without a device: the same per-lane code on host threads"""
    return _sha512_batch(None, msgs)


def _ed25519_verify_batch(ctx_handle, pks: bytes, msgs, sigs: bytes) -> bytes:
    n = len(msgs)
    if len(pks) != 32 * n or len(sigs) != 64 * n:
        raise BzkError("ed25519_verify_batch: pks must hold 32 and sigs 64 bytes per message")
    off, data = _offsets(msgs)
    ok = C.create_string_buffer(max(n, 1))
    _st(load_library().bzk_ed25519_verify_batch(ctx_handle, _ptr(pks) if n else None, _ptr(data), off, _ptr(sigs) if n else None, n, ok),
        "ed25519_verify_batch")
    return ok.raw[:n]


def host_ed25519_verify_batch(pks: bytes, msgs, sigs: bytes) -> bytes:
    """Bzk.ed25519_verify_batch without a device: the same per-lane code on host threads"""
    return _ed25519_verify_batch(None, pks, msgs, sigs)


ED25519_SIGN_ROUND = 1 << 16  # rows a host-pointer Ed25519 signing or key call stages per round (bzk_ed25519_sign.h ED25519_SIGN_ROUND)


def _ed25519_keys_batch(ctx_handle, seeds) -> bytes:
    n = len(seeds)
    off, data = _offsets(seeds)
    out = C.create_string_buffer(max(64 * n, 1))
    _st(load_library().bzk_ed25519_keys_batch(ctx_handle, _ptr(data), off, n, out), "ed25519_keys_batch")
    return out.raw[: 64 * n]


def _ed25519_sign_batch(ctx_handle, keys: bytes, msgs) -> bytes:
    n = len(msgs)
    if len(keys) != 64 * n:
        raise BzkError("ed25519_sign_batch: keys must hold 64 bytes per message")
    off, data = _offsets(msgs)
    sig = C.create_string_buffer(max(64 * n, 1))
    _st(load_library().bzk_ed25519_sign_batch(ctx_handle, _ptr(keys) if n else None, _ptr(data), off, n, sig), "ed25519_sign_batch")
    return sig.raw[: 64 * n]


def host_ed25519_keys_batch(seeds) -> bytes:
    """Bzk.ed25519_keys_batch without a device: the same per-lane code on host threads"""
    return _ed25519_keys_batch(None, seeds)


def host_ed25519_sign_batch(keys: bytes, msgs) -> bytes:
    """Bzk.ed25519_sign_batch without a device: the same per-lane code on host threads"""
    return _ed25519_sign_batch(None, keys, msgs)


def host_ed25519_keys(seed: bytes) -> bytes:
    """Ed25519::generate_keys(seed) on the host: secret | public"""
    out = C.create_string_buffer(64)
    _st(load_library().bzk_host_ed25519_keys(_ptr(seed) if seed else None, len(seed), out), "host_ed25519_keys")
    return out.raw


def host_ed25519_sign(keys: bytes, msg: bytes) -> bytes:
    """Ed25519::sign on the host: keys = secret | public, the signature R | s"""
    if len(keys) != 64:
        raise BzkError("host_ed25519_sign: keys is secret | public, 64 bytes")
    out = C.create_string_buffer(64)
    _st(load_library().bzk_host_ed25519_sign(_ptr(keys), _ptr(msg) if msg else None, len(msg), out), "host_ed25519_sign")
    return out.raw


def _signed_records(name: str, call, n: int, want_txs: bool, in_len: int):
    """runs call(sig, ok, txs_out, cap, out_len) with txs_out sized for every record gaining a signature"""
    lib = load_library()
    sig, ok = C.create_string_buffer(max(64 * n, 1)), C.create_string_buffer(max(n, 1))
    cap = in_len + 76 * n  # a record grows by at most a tag's change, a length prefix and the signature
    out = C.create_string_buffer(max(cap, 1)) if want_txs else None
    out_len = _u64(0)
    st = call(sig, ok, out, cap if want_txs else 0, C.byref(out_len))
    if st != 0:
        raise BzkError(f"{name}: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
    return sig.raw[: 64 * n], ok.raw[:n], (out.raw[: out_len.value] if want_txs else None)


def _mpn_deposits_sign(ctx_handle, keys: bytes, txs: bytes, n: int, want_txs: bool):
    if len(keys) != 64 * n:
        raise BzkError("mpn_deposits_sign: keys is not n x 64 bytes")
    lib = load_library()
    return _signed_records("mpn_deposits_sign", lambda sig, ok, out, cap, out_len: lib.bzk_mpn_deposits_sign(
        ctx_handle, _ptr(keys) if n else None, _ptr(txs) if txs else None, len(txs), n, sig, ok, out, cap, out_len), n, want_txs, len(txs))


def _l1_txs_sign(ctx_handle, keys: bytes, txs: bytes, n: int, form: int, want_hash: bool, want_txs: bool):
    if len(keys) != 64 * n:
        raise BzkError("l1_txs_sign: keys is not n x 64 bytes")
    lib = load_library()
    h = C.create_string_buffer(max(32 * n, 1)) if want_hash else None
    sig, ok, out = _signed_records("l1_txs_sign", lambda sig, ok, out, cap, out_len: lib.bzk_l1_txs_sign(
        ctx_handle, _ptr(keys) if n else None, _ptr(txs) if txs else None, len(txs), n, form, sig, ok, h, out, cap, out_len), n, want_txs, len(txs))
    return sig, ok, (h.raw[: 32 * n] if want_hash else None), out


def host_mpn_deposits_sign(keys: bytes, txs: bytes, n: int, want_txs: bool = True):
    """Bzk.mpn_deposits_sign without a device: the same per-lane code on host threads"""
    return _mpn_deposits_sign(None, keys, txs, n, want_txs)


def host_l1_txs_sign(keys: bytes, txs: bytes, n: int, form: int = L1_FORM_TX, want_hash: bool = True, want_txs: bool = True):
    """Bzk.l1_txs_sign without a device: the same per-lane code on host threads"""
    return _l1_txs_sign(None, keys, txs, n, form, want_hash, want_txs)


def _groth16_verify_batch(ctx_handle, vk_bincode: bytes, inputs: bytes, n_inputs: int, proofs: bytes) -> bytes:
    n = len(proofs) // 387
    if len(proofs) != 387 * n or len(inputs) != 32 * n_inputs * n:
        raise BzkError("groth16_verify_batch: proofs must hold 387 and inputs 32 n_inputs bytes per proof")
    ok = C.create_string_buffer(max(n, 1))
    _st(load_library().bzk_groth16_verify_batch(ctx_handle, _ptr(vk_bincode), len(vk_bincode), _ptr(inputs) if inputs else None, n_inputs,
                                                _ptr(proofs) if n else None, n, ok), "groth16_verify_batch")
    return ok.raw[:n]


def host_groth16_verify_batch(vk_bincode: bytes, inputs: bytes, n_inputs: int, proofs: bytes) -> bytes:
    """Bzk.groth16_verify_batch without a device: the same per-proof functions over the host field on host threads"""
    return _groth16_verify_batch(None, vk_bincode, inputs, n_inputs, proofs)


def _pack_keys(keys):
    """[(vk_bincode, n_inputs)] as the several-key entries take them: (the keys' bytes back to back, vk_off of len + 1, n_inputs)"""
    off = [0]
    for vk, _ in keys:
        off.append(off[-1] + len(vk))
    return (b"".join(vk for vk, _ in keys), (C.c_uint64 * len(off))(*off), (C.c_uint32 * max(len(keys), 1))(*[k for _, k in keys]))


def _groth16_verify_batch_keys(ctx_handle, keys, key_of, inputs: bytes, proofs: bytes) -> bytes:
    n = len(proofs) // 387
    if len(proofs) != 387 * n or len(key_of) != n:
        raise BzkError("groth16_verify_batch_keys: proofs must hold 387 bytes and key_of one index per proof")
    per_key = collections.Counter(key_of)   # key_of: a sequence of ints, or a ctypes array of c_uint32 (passed as it is)
    if all(0 <= k < len(keys) for k in per_key) and len(inputs) != sum(32 * keys[k][1] * c for k, c in per_key.items()):
        raise BzkError("groth16_verify_batch_keys: inputs must hold 32 n_inputs[key_of[i]] bytes per proof")
    vks, vk_off, n_inputs = _pack_keys(keys)
    ok = C.create_string_buffer(max(n, 1))
    _st(load_library().bzk_groth16_verify_batch_keys(ctx_handle, len(keys), _ptr(vks) if vks else None, vk_off, n_inputs,
                                                     key_of if isinstance(key_of, C.Array) else (C.c_uint32 * max(n, 1))(*key_of),
                                                     _ptr(inputs) if inputs else None,
                                                     _ptr(proofs) if n else None, n, ok), "groth16_verify_batch_keys")
    return ok.raw[:n]


def host_groth16_verify_batch_keys(keys, key_of, inputs: bytes, proofs: bytes) -> bytes:
    """Bzk.groth16_verify_batch_keys without a device: the same per-proof functions over the host field, all proofs in one task loop"""
    return _groth16_verify_batch_keys(None, keys, key_of, inputs, proofs)


def _subgroup_check_batch(ctx_handle, group: str, pts: bytes, inf: bytes = None) -> bytes:
    size = {"g1": 96, "g2": 192}[group]
    n = len(pts) // size
    if len(pts) != size * n or (inf is not None and len(inf) != n):
        raise BzkError("subgroup_check_batch: pts must hold %d bytes per point and inf one flag per point" % size)
    lib = load_library()
    fn = {"g1": lib.bzk_g1_subgroup_check_batch, "g2": lib.bzk_g2_subgroup_check_batch}[group]
    ok = C.create_string_buffer(max(n, 1))
    _st(fn(ctx_handle, _ptr(pts) if n else None, _ptr(inf) if inf else None, n, ok), "subgroup_check_batch")
    return ok.raw[:n]


def _bellman_params_check(ctx_handle, blob: bytes):
    report = (C.c_uint64 * 4)()
    st = load_library().bzk_bellman_params_check(ctx_handle, _ptr(blob), len(blob), report)
    if st < 0:
        _st(st, "bellman_params_check")
    return st, tuple(report)


def _h(ctx):
    return ctx.h if ctx is not None else None


def g1_scale_batch(ctx, pts: bytes, k: bytes):
    """(out, inf): out[i] = k * pts[i] for raw 96-byte G1 points of the order-r subgroup, k one 32-byte Montgomery Fr scalar; an identity result is 96
    zero bytes with inf[i] = 1.  ctx: a Bzk (one GPU lane per point) or None (host threads)"""
    n = len(pts) // 96
    if len(pts) != 96 * n or len(k) != 32:
        raise BzkError("g1_scale_batch: pts must hold 96 bytes per point and k 32 bytes")
    out, inf = C.create_string_buffer(max(96 * n, 1)), C.create_string_buffer(max(n, 1))
    _st(load_library().bzk_g1_scale_batch(_h(ctx), _ptr(pts) if n else None, n, _ptr(k), out, inf), "g1_scale_batch")
    return out.raw[: 96 * n], inf.raw[:n]


def params_rekey(ctx, ph, d: bytes):
    """(new params handle, its 870-byte vk head): bzk_params_rekey - needs a context"""
    if len(d) != 32:
        raise BzkError("params_rekey: d must hold 32 bytes")
    h, vk = C.c_void_p(), C.create_string_buffer(870)
    _st(load_library().bzk_params_rekey(_h(ctx), ph, _ptr(d), C.byref(h), vk), "params_rekey")
    return h, vk.raw


def bellman_params_rekey(ctx, blob: bytes, d: bytes) -> bytes:
    """the bellman `Parameters` blob with delta times d (h and l times 1 / d); ctx None: host threads - the same bytes either way"""
    if len(d) != 32:
        raise BzkError("bellman_params_rekey: d must hold 32 bytes")
    lib, n = load_library(), _u64()
    _st(lib.bzk_bellman_params_rekey(_h(ctx), _ptr(blob), len(blob), _ptr(d), None, 0, C.byref(n)), "bellman_params_rekey")
    out = C.create_string_buffer(max(n.value, 1))
    _st(lib.bzk_bellman_params_rekey(_h(ctx), _ptr(blob), len(blob), _ptr(d), out, n.value, None), "bellman_params_rekey")
    return out.raw[: n.value]


def bellman_params_rekey_check(ctx, before: bytes, after: bytes, seed: bytes):
    """(verdict, report): is `after` a re-key of `before` by some d - 1 or 0 with report = (array, index, code, 0) of the first failure.  The verdict
    is only as good as the secrecy of `seed` (32 bytes) from whoever made `after`"""
    if len(seed) != 32:
        raise BzkError("bellman_params_rekey_check: seed must hold 32 bytes")
    report = (C.c_uint64 * 4)()
    st = load_library().bzk_bellman_params_rekey_check(_h(ctx), _ptr(before), len(before), _ptr(after), len(after), _ptr(seed), report)
    if st < 0:
        _st(st, "bellman_params_rekey_check")
    return st, tuple(report)


_POINT_BYTES = {"g1": 96, "g2": 192}


def mul_batch(ctx, group: str, pts: bytes, scalars: bytes, canonical: bool = False):
    """(out, inf): out[i] = scalars[i] * pts[i] for raw G1 (96-byte) or G2 (192-byte) points of the order-r subgroup; scalars 32 bytes each, Montgomery
    limbs or, with canonical, plain integers; an identity result is zero bytes with inf[i] = 1.  ctx: a Bzk (one GPU lane per point) or None (host threads)"""
    size = _POINT_BYTES[group]
    n = len(pts) // size
    if len(pts) != size * n or len(scalars) != 32 * n:
        raise BzkError("mul_batch: pts must hold %d bytes per point and scalars 32" % size)
    lib = load_library()
    fn = {"g1": lib.bzk_g1_mul_batch, "g2": lib.bzk_g2_mul_batch}[group]
    out, inf = C.create_string_buffer(max(size * n, 1)), C.create_string_buffer(max(n, 1))
    _st(fn(_h(ctx), _ptr(pts) if n else None, _ptr(scalars) if n else None, n, BZK_F_CANONICAL if canonical else 0, out, inf), "mul_batch")
    return out.raw[: size * n], inf.raw[:n]


def mul_powers(ctx, group: str, pts: bytes, c: bytes, s: bytes, start: int = 0):
    """(out, inf): out[i] = c * s^(start + i) * pts[i]; c and s 32-byte Montgomery Fr scalars, treated as secrets by the library"""
    size = _POINT_BYTES[group]
    n = len(pts) // size
    if len(pts) != size * n or len(c) != 32 or len(s) != 32:
        raise BzkError("mul_powers: pts must hold %d bytes per point, c and s 32 bytes" % size)
    lib = load_library()
    fn = {"g1": lib.bzk_g1_mul_powers, "g2": lib.bzk_g2_mul_powers}[group]
    out, inf = C.create_string_buffer(max(size * n, 1)), C.create_string_buffer(max(n, 1))
    _st(fn(_h(ctx), _ptr(pts) if n else None, n, _ptr(c), _ptr(s), start, out, inf), "mul_powers")
    return out.raw[: size * n], inf.raw[:n]


def ptau_size(log_m: int) -> int:
    return load_library().bzk_ptau_size(log_m)


def ptau_init(log_m: int) -> bytes:
    """the trivial powers-of-tau accumulator for m = 2^log_m: every entry its group's generator"""
    n = ptau_size(log_m)
    if n == 0:
        raise BzkError("ptau_init: log_m must be 1 .. 24")
    out = C.create_string_buffer(n)
    _st(load_library().bzk_ptau_init(log_m, out, n), "ptau_init")
    return out.raw


def ptau_contribute(ctx, blob: bytes, secrets: bytes):
    """(new accumulator, key): `blob` with tau, alpha, beta multiplied by secrets = tau | alpha | beta (3 x 32 bytes Montgomery, none zero); key = tau G2 |
    alpha G2 | beta G2 (576 bytes).  ctx None: host threads - the same bytes either way"""
    if len(secrets) != 96:
        raise BzkError("ptau_contribute: secrets must hold 96 bytes")
    out, key = C.create_string_buffer(max(len(blob), 1)), C.create_string_buffer(576)
    _st(load_library().bzk_ptau_contribute(_h(ctx), _ptr(blob), len(blob), _ptr(secrets), out, len(blob), key), "ptau_contribute")
    return out.raw[: len(blob)], key.raw


def ptau_check(ctx, before, key, after: bytes, seed: bytes):
    """(verdict, report): is `after` a well-formed accumulator and, with before and key (both or neither), one contribution on top of `before` - 1 or 0
    with report = (array, index, code, 0) of the first failure.  The verdict is only as good as the secrecy of `seed` (32 bytes) from whoever made `after`"""
    if len(seed) != 32 or (before is None) != (key is None) or (key is not None and len(key) != 576):
        raise BzkError("ptau_check: seed must hold 32 bytes, key 576; before and key come together")
    report = (C.c_uint64 * 4)()
    st = load_library().bzk_ptau_check(_h(ctx), _ptr(before) if before is not None else None, len(before) if before is not None else 0,
                                       _ptr(key) if key is not None else None, _ptr(after), len(after), _ptr(seed), report)
    if st < 0:
        _st(st, "ptau_check")
    return st, tuple(report)


def host_bellman_params_check(blob: bytes):
    """Bzk.bellman_params_check without a device: the whole check on host threads"""
    return _bellman_params_check(None, blob)


def host_subgroup_check_batch(group: str, pts: bytes, inf: bytes = None) -> bytes:
    """Bzk.subgroup_check_batch without a device: the same per-point functions over the host field on host threads"""
    return _subgroup_check_batch(None, group, pts, inf)


def host_sha512(b: bytes) -> bytes:
    out = C.create_string_buffer(64)
    _st(load_library().bzk_host_sha512(_ptr(b) if b else None, len(b), out), "host_sha512")
    return out.raw


def host_ed25519_verify(pk: bytes, msg: bytes, sig: bytes) -> bool:
    r = load_library().bzk_host_ed25519_verify(_ptr(pk), _ptr(msg) if msg else None, len(msg), _ptr(sig))
    if r < 0:
        raise BzkError("ed25519_verify: bad argument")
    return bool(r)


def _mpn_deposit_verify_batch(ctx_handle, txs: bytes, n: int, want_address: bool):
    lib = load_library()
    ok = C.create_string_buffer(max(n, 1))
    xy = C.create_string_buffer(max(64 * n, 1)) if want_address else None
    st = lib.bzk_mpn_deposit_verify_batch(ctx_handle, _ptr(txs), len(txs), n, ok, xy)
    if st != 0:
        raise BzkError(f"mpn_deposit_verify_batch: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
    return ok.raw[:n], (xy.raw[: 64 * n] if want_address else None)


def host_mpn_deposit_verify_batch(txs: bytes, n: int, want_address: bool = True):
    """Bzk.mpn_deposit_verify_batch without a device: the same verdicts and addresses on host threads"""
    return _mpn_deposit_verify_batch(None, txs, n, want_address)


def mpn_set_wire_flags(flags: int):
    """process-wide: WORK_SIG_LEN_PREFIXED where wire-form deposits carry length-prefixed Ed25519 signatures (ed25519 < 1.3), else 0"""
    _st(load_library().bzk_mpn_set_wire_flags(flags), "mpn_set_wire_flags")


def _l1_tx_verify_batch(ctx_handle, txs: bytes, n: int, form: int, want_hash: bool):
    lib = load_library()
    ok = C.create_string_buffer(max(n, 1))
    h = C.create_string_buffer(max(32 * n, 1)) if want_hash else None
    st = lib.bzk_l1_tx_verify_batch(ctx_handle, _ptr(txs) if txs else None, len(txs), n, form, ok, h)
    if st != 0:
        raise BzkError(f"l1_tx_verify_batch: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
    return ok.raw[:n], (h.raw[: 32 * n] if want_hash else None)


def host_l1_tx_verify_batch(txs: bytes, n: int, form: int = L1_FORM_TX, want_hash: bool = True):
    """Bzk.l1_tx_verify_batch without a device: the same per-lane code on host threads"""
    return _l1_tx_verify_batch(None, txs, n, form, want_hash)


def _sha3_merkle_roots(ctx_handle, leaves: bytes, counts, want_nodes: bool):
    m = len(counts)
    if len(leaves) != 32 * sum(counts):
        raise BzkError("sha3_merkle_roots: leaves must hold 32 bytes per counted leaf")
    cnt = (C.c_uint64 * max(m, 1))(*counts)
    n_nodes = sum(max(1, 2 * c - 1) for c in counts)
    roots = C.create_string_buffer(max(32 * m, 1))
    nodes = C.create_string_buffer(max(32 * n_nodes, 1)) if want_nodes else None
    _st(load_library().bzk_sha3_merkle_roots(ctx_handle, _ptr(leaves) if leaves else None, cnt, m, roots, nodes), "sha3_merkle_roots")
    return (roots.raw[: 32 * m], nodes.raw[: 32 * n_nodes]) if want_nodes else roots.raw[: 32 * m]


def host_sha3_merkle_roots(leaves: bytes, counts, want_nodes: bool = False):
    """Bzk.sha3_merkle_roots without a device"""
    return _sha3_merkle_roots(None, leaves, counts, want_nodes)


def _block_bodies_check(ctx_handle, txs: bytes, counts, want_tx: bool):
    lib = load_library()
    m, n = len(counts), sum(counts)
    cnt = (C.c_uint64 * max(m, 1))(*counts)
    sig_ok = C.create_string_buffer(max(m, 1))
    roots = C.create_string_buffer(max(32 * m, 1))
    tx_ok = C.create_string_buffer(max(n, 1)) if want_tx else None
    h = C.create_string_buffer(max(32 * n, 1)) if want_tx else None
    st = lib.bzk_block_bodies_check(ctx_handle, _ptr(txs) if txs else None, len(txs), cnt, m, sig_ok, roots, tx_ok, h)
    if st != 0:
        raise BzkError(f"block_bodies_check: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
    return sig_ok.raw[:m], roots.raw[: 32 * m], (tx_ok.raw[:n] if want_tx else None), (h.raw[: 32 * n] if want_tx else None)


def host_block_bodies_check(txs: bytes, counts, want_tx: bool = True):
    """Bzk.block_bodies_check without a device"""
    return _block_bodies_check(None, txs, counts, want_tx)


UPD_PROOF, UPD_SIGS, UPD_ROUTE, UPD_UNSUPPORTED = 1, 2, 4, 0x80   # bzk_contract_updates_check's verdict bits


class _ContractFn(C.Structure):
    _fields_ = [("vk", C.c_void_p), ("vk_len", C.c_uint64), ("log4_payment_capacity", C.c_uint8)]


class _ContractDescStruct(C.Structure):
    _fields_ = [("contract_id", C.c_uint8 * 32), ("deposit_fns", C.c_void_p), ("n_deposit_fns", C.c_uint32), ("withdraw_fns", C.c_void_p),
                ("n_withdraw_fns", C.c_uint32), ("fns", C.c_void_p), ("n_fns", C.c_uint32)]


class ContractDesc:
    """bzk_contract_desc: contract_id = the 32 Montgomery bytes of the ContractId's scalar; deposit_fns / withdraw_fns = [(bincode(Groth16VerifyingKey),
    log4_payment_capacity)], fns = [bincode(Groth16VerifyingKey)].  Keeps the key bytes alive as long as it lives."""

    def __init__(self, contract_id: bytes, deposit_fns=(), withdraw_fns=(), fns=()):
        assert len(contract_id) == 32
        self._keep = []
        self.c = _ContractDescStruct()
        self.c.contract_id[:] = contract_id
        for name, table in (("deposit_fns", list(deposit_fns)), ("withdraw_fns", list(withdraw_fns)), ("fns", [(vk, 0) for vk in fns])):
            arr = (_ContractFn * max(len(table), 1))()
            for k, (vk, cap) in enumerate(table):
                buf = C.create_string_buffer(bytes(vk), len(vk))
                self._keep.append(buf)
                arr[k].vk, arr[k].vk_len, arr[k].log4_payment_capacity = C.addressof(buf), len(vk), cap
            self._keep.append(arr)
            setattr(self.c, name, C.addressof(arr))
            setattr(self.c, "n_" + name, len(table))


def _contract_updates_check(ctx_handle, contract: ContractDesc, updates: bytes, counts, height0: int, state0: bytes):
    lib = load_library()
    m, n = len(counts), sum(counts)
    cnt = (C.c_uint64 * max(m, 1))(*counts)
    ok = C.create_string_buffer(max(n, 1))
    aux = C.create_string_buffer(max(32 * n, 1))
    commit = C.create_string_buffer(max(32 * n, 1))
    st = lib.bzk_contract_updates_check(ctx_handle, C.byref(contract.c), _ptr(updates) if updates else None, len(updates), cnt, m, height0,
                                        _ptr(state0), ok, aux, commit)
    if st != 0:
        raise BzkError(f"contract_updates_check: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
    return ok.raw[:n], aux.raw[: 32 * n], commit.raw[: 32 * n]


def host_contract_updates_check(contract: ContractDesc, updates: bytes, counts, height0: int, state0: bytes):
    """Bzk.contract_updates_check without a device: the same per-lane functions on host threads"""
    return _contract_updates_check(None, contract, updates, counts, height0, state0)


def l1_tx_updates(txs: bytes, n: int, contract_id: bytes, form: int = L1_FORM_TX, cap=None):
    """host only: (found, [(transaction index, offset, length)]) of every ContractUpdate of every UpdateContract of contract_id among n
    Transaction / TransactionAndDelta records; at most cap spans are returned (None: all of them)"""
    lib = load_library()
    found = C.c_uint64(0)

    def call(k):
        spans = (C.c_uint64 * max(3 * k, 1))()
        st = lib.bzk_l1_tx_updates(_ptr(txs) if txs else None, len(txs), n, form, _ptr(contract_id), spans, k, C.byref(found))
        if st != 0:
            raise BzkError(f"l1_tx_updates: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
        return [tuple(spans[3 * i:3 * i + 3]) for i in range(min(k, found.value))]
    out = call(0 if cap is None else cap)
    if cap is None and found.value:
        out = call(found.value)
    return found.value, out


def l1_tx_deltas(txs: bytes, n: int, contract_id: bytes, form: int = L1_FORM_TX, cap=None):
    """host only: (found, [(transaction index, offset of the ZkDeltaPairs body, length, source)]) for every UpdateContract of contract_id among
    n Transaction / TransactionAndDelta records - source 0: the transaction's `delta`, 1: the record's `state_delta`, 2 (length 0): neither;
    at most cap spans are returned (None: all of them)"""
    lib = load_library()
    found = C.c_uint64(0)

    def call(k):
        spans = (C.c_uint64 * max(4 * k, 1))()
        st = lib.bzk_l1_tx_deltas(_ptr(txs) if txs else None, len(txs), n, form, _ptr(contract_id), spans, k, C.byref(found))
        if st != 0:
            raise BzkError(f"l1_tx_deltas: {lib.bzk_strerror(st).decode()} [{lib.bzk_mpn_work_last_error().decode()}]")
        return [tuple(spans[4 * i:4 * i + 4]) for i in range(min(k, found.value))]
    out = call(0 if cap is None else cap)
    if cap is None and found.value:
        out = call(found.value)
    return found.value, out
