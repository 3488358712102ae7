// What pmul.hip (n points times n scalars) and ptau.hip (the powers-of-tau accumulator on top of it) share with each other and with rekey.hip: the one
// multiplication call every entry point goes through, and the host pieces of a seeded check (generators, rho, the seeded sum, the pairing product).
#pragma once
#include <string.h>

#include <vector>

#include "bzk_curve.cuh"
#include "bzk_rekey.h"
#include "host_pairing.h"
#include "host_threads.h"

namespace bzk {

// pmul.hip: out[i] = k_i pts[i] for n raw records (96 bytes on G1, 192 on G2).  k_i = scalars[i] (32 bytes each; canonical: plain integers, else
// Montgomery limbs), or, where scalars is null, c s^(start + i) for the Montgomery scalars c and s.  ctx = NULL: host pointers, host threads.
// on_device: pts / scalars / out / inf are device pointers (out may be pts), else host pointers staged in rounds.  inf may be null.
// BZK_E_ARG, nothing written: a scalar (or c, s) whose limbs are not below r.  The rows of the recoded scalars and the table of powers are
// overwritten on the device, c, s and the table on the host, before the call returns
struct PmCall {
    bool g2 = false;
    const uint8_t* pts = nullptr;
    bool on_device = false;
    uint64_t n = 0;
    const uint8_t* scalars = nullptr;
    bool canonical = false;
    const uint8_t *c = nullptr, *s = nullptr;
    uint64_t start = 0;
    uint8_t* out = nullptr;
    uint8_t* inf = nullptr;
};
int32_t pm_run(bzk_ctx* ctx, const char* who, const PmCall& call);

// rekey.hip: the standard generators, e(a, q1) == e(b, q2), and rho_i = the low 16 bytes of SHA3-256(seed | code | LE64(i)) as a canonical
// 32-byte integer
hp::G1A g1_gen();
hp::G2A g2_gen();
bool pairings_equal(const hp::G1A& a, const hp::G2A& q1, const hp::G1A& b, const hp::G2A& q2);
void rho_of(const uint8_t seed[32], uint8_t code, uint64_t i, uint8_t out32[32]);

// k P on the host for a canonical k of `bits` bits, generic XYZZ (a handful of points per call: a head's delta_g2, the terms of a host sum)
template <class F>
XyzzT<F> host_mul(const AffineT<F>& p, const uint32_t* k, int bits) {
    XyzzT<F> r = xyzz_identity<F>();
    for (int i = bits - 1; i >= 0; --i) {
        r = xyzz_dbl<F>(r);
        if ((k[i >> 5] >> (i & 31)) & 1) xyzz_add_mixed<F>(r, p);
    }
    return r;
}

// S = sum_i rho_i q_i over n raw records of sizeof(AffineT<F>) bytes on host threads: every chunk its own running sum, the chunks' sums added at
// the end.  False: S is the identity
template <class F>
bool host_seeded_sum(const uint8_t* q, uint64_t n, const uint8_t seed[32], uint8_t code, AffineT<F>& out) {
    typedef XyzzT<F> Pt;
    const uint64_t chunk = 256, n_chunks = (n + chunk - 1) / chunk;
    std::vector<Pt> part(n_chunks, xyzz_identity<F>());
    host_for_each(n_chunks, host_default_threads(), [&](uint64_t c) {
        Pt acc = xyzz_identity<F>();
        for (uint64_t i = c * chunk; i < n && i < (c + 1) * chunk; ++i) {
            uint8_t rho[32];
            uint32_t k[8];
            rho_of(seed, code, i, rho);
            memcpy(k, rho, 32);
            AffineT<F> p;
            memcpy(&p, q + sizeof p * i, sizeof p);
            xyzz_add<F>(acc, host_mul<F>(p, k, 128));
        }
        part[c] = acc;
    });
    Pt s = xyzz_identity<F>();
    for (const Pt& p : part) xyzz_add<F>(s, p);
    return xyzz_to_affine<F>(s, out);
}

}  // namespace bzk
