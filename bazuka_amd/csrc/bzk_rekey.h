// What rekey.hip shares with groth16.hip and host_bellman.hip: the scaling of a G1 array by one recoded scalar, wherever the array lies, and the
// hooks a re-key of a resident key or of a bellman blob needs from the units that own those forms.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/bzk.h"

namespace bzk {

// overwrites n bytes through a volatile pointer (a secret's host copy: the store must not be optimised away)
inline void wipe_host(void* p, size_t n) {
    volatile uint8_t* v = (volatile uint8_t*)p;
    for (size_t i = 0; i < n; ++i) v[i] = 0;
}

// rekey.hip: out[i] = k pts[i] for n raw 96-byte records, k one Montgomery Fr scalar (BZK_E_ARG: limbs not below r).  ctx = NULL: host pointers, host
// threads.  on_device: pts / out / inf are device pointers (out may be pts), else host pointers staged in rounds.  inf may be null.  The recoded
// scalar is overwritten on the host and on the device before the call returns
int32_t g1_scale_run(bzk_ctx* ctx, const char* who, const uint8_t* pts, bool on_device, uint64_t n, const uint8_t k[32], uint8_t* out, uint8_t* inf);

// groth16.hip: a new handle of src's shape and densities whose five arrays are allocated and not filled, its vk a copy of src's; dev[k] = the new
// handle's h, l, a, b_g1, b_g2 and src_dev[k] the source's, n[k] their point counts
int32_t params_clone_shape(bzk_ctx* ctx, const bzk_params* src, bzk_params** out, void* dev[5], const void* src_dev[5], uint64_t n[5]);


// rekey.hip, for the two re-key entry points (a resident key there, a bellman blob in host_bellman.hip).
// rekey_scalars: d (Montgomery) -> dinv = d^-1; BZK_E_ARG when d is zero or its limbs are not below r.  The caller wipes dinv
int32_t rekey_scalars(const uint8_t d[32], uint8_t dinv[32]);
// delta_g1 and delta_g2 of a packed 870-byte head times d, on the host
void rekey_vk_head(uint8_t vk870[870], const uint8_t d[32]);
// e(delta_g1, G2) == e(G1, delta_g2) for the head's two deltas
bool rekey_delta_consistent(const uint8_t vk870[870]);
// *holds = ( e(S(after), delta_g2 of vk_after) == e(S(before), delta_g2 of vk_before) ),  S(q) = sum_i rho_i q_i over n raw records,
// rho_i = the low 16 bytes of SHA3-256(seed | code | LE64(i)).  The two sums: device MSMs with a context, host threads without
int32_t rekey_ratio(bzk_ctx* ctx, uint8_t code, const uint8_t* before, const uint8_t* after, uint64_t n, const uint8_t seed[32],
                    const uint8_t vk_before[870], const uint8_t vk_after[870], bool* holds);

}  // namespace bzk
