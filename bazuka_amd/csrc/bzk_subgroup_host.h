// The host's base field (host_fp64.h: 6 x 64-bit limbs, values canonical) under the policy interface of bzk_subgroup.cuh: what the ctx = NULL paths
// of subgroup.hip and rekey.hip run the per-point functions over.  Host code only.
#pragma once
#include <string.h>

#include "bzk_subgroup.cuh"
#include "host_fp64.h"

namespace bzk {

struct SgHFp {
    typedef HFp T;
    static T zero() { return HFpOps::zero(); }
    static T one() { return HFpOps::one(); }
    static bool is_zero(const T& a) { return HFpOps::is_zero(a); }  // canonical values: a limb test
    static T add(const T& a, const T& b) { return HFpOps::add(a, b); }
    static T sub(const T& a, const T& b) { return HFpOps::sub(a, b); }
    static T mul(const T& a, const T& b) { return HFpOps::mul(a, b); }
    static T sqr(const T& a) { return HFpOps::mul(a, a); }
    static T mul12(const T& a) {
        const T a3 = HFpOps::add(HFpOps::dbl(a), a);
        return HFpOps::dbl(HFpOps::dbl(a3));
    }
    static T cst(const fp28::Consts& c) {  // the 28-bit Montgomery-2^392 constant as canonical Montgomery-2^384 limbs
        const Fp f = fp28::from28(fp28::consts_as_fp28(c));
        T r;
        memcpy(r.l, f.l, 48);
        return r;
    }
    static bool load(const uint32_t* w, T& out) {
        memcpy(out.l, w, 48);
        return !hfp::geq_p(out.l, hfp::consts().p);
    }
    // bzk_scale.cuh
    static T inv(const T& a) { return HFpOps::inv(a); }  // 0 -> 0
    static void store(const T& a, uint32_t* w) { memcpy(w, a.l, 48); }
};

}  // namespace bzk
