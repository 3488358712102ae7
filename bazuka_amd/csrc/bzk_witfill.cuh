// Witness value traces on the device (round 5): the part of an MPN circuit's assignment that hangs off Poseidon
// outputs - the Poseidon gadget's own S-box / idle-lane variables (2/3 of a transition's constraints), the Merkle gadget's muxes,
// the equality checks against computed roots - is not evaluated by the host generator but DEFERRED: the gadgets of host_r1cs.h emit
// a small program per transition instead (the same for every transition of a circuit shape) plus a record of the values the host does
// know, leave the slots of z / A.z / B.z / C.z untouched, and the device fills them in after the arrays have been uploaded.
//
//   reference gadgets whose VALUE semantics the ops restate (allocation order and the three values per constraint as the host forms do):
//     Poseidon gadget      /root/reference/src/zk/groth16/gadgets/poseidon/mod.rs:8-95     F_POSEIDON (trace), V_HASH (output only)
//     mux                  /root/reference/src/zk/groth16/gadgets/common/mux.rs:7-47       F_MUX, V_SEL
//     assert_equal(_if_enabled)  .../common/number.rs:121-177                               F_ENFORCE_EQ, F_ASSERT_EQ_IF
//
// Two passes.  Pass 1 (V ops, by dependency level: a Merkle path is a chain of hashes): registers = the deferred VALUES, one 32-byte
// Montgomery-256 scalar per (register, transition), computed with the sparse-partial-round hash of bzk_poseidon29.cuh.  Pass 2 (F ops, all
// independent once the registers are known: one lane per (op, transition)): the slots.  The dense intermediate states the gadget allocates are
// only produced here, in pass 2 - the sparse form skips them.  Everything is BZK_HD: the CPU harness and bzk_r1cs_fill_host run the same code.
#pragma once
#include "bzk_fr29.cuh"
#include "bzk_poseidon29.cuh"

namespace bzk {
namespace wf {

enum : uint8_t { V_HASH = 1, V_SEL = 2, F_POSEIDON = 3, F_MUX = 4, F_ASSERT_EQ_IF = 5, F_ENFORCE_EQ = 6, F_CHECK_EQ = 7, V_LADDER = 8, F_LADDER = 9 };
constexpr int MAX_SEL_CHAIN = 8;  // links operand() follows on the device; DeferProgram::finalize measures a program's, witfill_run_dev refuses deeper ones
enum : uint32_t { FLAG_UNSATISFIED = 1u, FLAG_CHAIN = 2u };  // a deferred constraint does not hold / a computed state differs from the builder's prediction

// operand: >= 0 a register, < 0 ~index into the transition's input record
struct Op {
    uint8_t kind;
    uint8_t t;        // V_HASH / F_POSEIDON: state width (arity + 1); V_SEL / F_MUX: 0 = Boolean::Is, 1 = Boolean::Not
    uint16_t level;   // V_HASH: 1 + the highest level among the producers of its register operands; V_SEL: that highest level itself
    int32_t out;      // V ops: the register written; F ops: unused (-1)
    uint32_t aux_off, con_off;  // F ops: first variable / constraint slot inside the transition's window
    int32_t in[7];
};

// counts of the Poseidon gadget for width t (arity t - 1): three variables and constraints per S-box, one per idle lane of a partial round
BZK_HD uint32_t poseidon_slots(int t, int rf, int rp) { return (uint32_t)(rf * t * 3 + rp * (3 + (t - 1))); }

struct Arrays {       // device (or host) views of the assignment; the aux part of z starts at z_aux
    Fr* z_aux;
    Fr* az;
    Fr* bz;
    Fr* cz;
};
struct TxView {       // where transition `tx` lives
    const Fr* inputs; // its input record
    Fr* regs;         // regs[r * reg_stride]
    size_t reg_stride;
    size_t aux_base, con_base;
    // device: per register {select input, a, b, Is / Not} of the V_SEL that defines it, or {.., .., .., -1}: selections are then never
    // materialised - an operand that names one is resolved here, through at most a few links (a Merkle level is two deep), which
    // takes the ~35 one-select launches out of pass 1.  nullptr (host executor): every V_SEL has been executed into its register
    const int32_t* sel;
};

BZK_HD Fr operand(const TxView& v, int32_t o) {
    if (v.sel) {
        for (int it = 0; it < MAX_SEL_CHAIN && o >= 0; ++it) {
            const int32_t* s = v.sel + 4 * (size_t)o;
            if (s[3] < 0) break;
            const bool bit = !v.inputs[~s[0]].is_zero();
            o = (s[3] == 0 ? bit : !bit) ? s[2] : s[1];
        }
    }
    return o >= 0 ? v.regs[(size_t)o * v.reg_stride] : v.inputs[~o];
}
BZK_HD Fr fr_one_mont() { return Fr::one(); }

// ---- pass 1 -------------------------------------------------------------------------------------------------------------------
template <int T>
BZK_HD void v_hash(const Op& op, const TxView& v, const Fr29* __restrict__ sparse_consts, int rf, int rp) {
    Fr in[T - 1];
#pragma unroll
    for (int i = 0; i < T - 1; ++i) in[i] = operand(v, op.in[i]);
    v.regs[(size_t)op.out * v.reg_stride] = poseidon29_hash<T>(in, sparse_consts, rf, rp);
}
// in[0] = the select bit's VALUE (an input: 0 / 1 in Montgomery form), in[1] = a, in[2] = b.   Is: bit ? b : a.   Not: bit ? a : b
BZK_HD void v_sel(const Op& op, const TxView& v) {
    const bool bit = !operand(v, op.in[0]).is_zero();
    const bool take_b = op.t == 0 ? bit : !bit;
    v.regs[(size_t)op.out * v.reg_stride] = operand(v, take_b ? op.in[2] : op.in[1]);
}

// ---- pass 2 -------------------------------------------------------------------------------------------------------------------
// dense constants of width T in the 29-bit form: rc[(rf + rp) * T] | mds[T * T]
template <int T>
BZK_HD void f_poseidon(const Op& op, const TxView& v, const Arrays& A, const Fr29* __restrict__ dense, int rf, int rp) {
    Fr29 e[T];
    e[0] = fr29::zero();
#pragma unroll
    for (int i = 1; i < T; ++i) e[i] = fr29::to29(operand(v, op.in[i - 1]));
    size_t a = v.aux_base + op.aux_off, c = v.con_base + op.con_off;
    const Fr one = fr_one_mont();
    const Fr29* mds = dense + (size_t)(rf + rp) * T;
    auto sbox = [&](const Fr29& x) {  // x2 = x x, x4 = x2 x2, x5 = x x4: three variables, three constraints
        const Fr29 x2 = fr29::sqr(x), x4 = fr29::sqr(x2), x5 = fr29::mul(x, x4);
        const Fr X = fr29::from29(x), X2 = fr29::from29(x2), X4 = fr29::from29(x4), X5 = fr29::from29(x5);
        A.z_aux[a] = X2; A.z_aux[a + 1] = X4; A.z_aux[a + 2] = X5;
        A.az[c] = X;  A.bz[c] = X;  A.cz[c] = X2;
        A.az[c + 1] = X2; A.bz[c + 1] = X2; A.cz[c + 1] = X4;
        A.az[c + 2] = X;  A.bz[c + 2] = X4; A.cz[c + 2] = X5;
        a += 3; c += 3;
        return x5;
    };
#pragma unroll 1
    for (int rnd = 0; rnd < rf + rp; ++rnd) {
        const Fr29* rc = dense + (size_t)rnd * T;
#pragma unroll
        for (int i = 0; i < T; ++i) e[i] = fr29::norm(fr29::add(e[i], rc[i]));  // k <= 3
        const bool full = rnd < rf / 2 || rnd >= rf / 2 + rp;
        if (full) {
#pragma unroll
            for (int i = 0; i < T; ++i) e[i] = sbox(e[i]);
        } else {
            e[0] = sbox(e[0]);
#pragma unroll
            for (int i = 1; i < T; ++i) {  // Number::compress: v * 1 = v
                const Fr V = fr29::from29(e[i]);
                A.z_aux[a] = V;
                A.az[c] = V; A.bz[c] = one; A.cz[c] = V;
                ++a; ++c;
            }
        }
        Fr29 nw[T];
#pragma unroll
        for (int j = 0; j < T; ++j) nw[j] = p29::row_dot<T>(mds + j * T, e);
#pragma unroll
        for (int j = 0; j < T; ++j) e[j] = nw[j];
    }
}
// select ? b : a, one variable, one constraint.  Is:  (a - b) * bit = a - ret.   Not: ret = bit ? a : b,  (b - a) * bit = b - ret
BZK_HD void f_mux(const Op& op, const TxView& v, const Arrays& A) {
    const Fr s = operand(v, op.in[0]), x = operand(v, op.in[1]), y = operand(v, op.in[2]);
    const bool bit = !s.is_zero();
    const size_t a = v.aux_base + op.aux_off, c = v.con_base + op.con_off;
    if (op.t == 0) {
        const Fr ret = bit ? y : x;
        A.z_aux[a] = ret;
        A.az[c] = fe_sub<FrParams>(x, y); A.bz[c] = s; A.cz[c] = fe_sub<FrParams>(x, ret);
    } else {
        const Fr ret = bit ? x : y;
        A.z_aux[a] = ret;
        A.az[c] = fe_sub<FrParams>(y, x); A.bz[c] = s; A.cz[c] = fe_sub<FrParams>(y, ret);
    }
}
// in[0] = enabled (bit value), in[1] = this, in[2] = other:  eis = enabled ? this : 0;  enabled * this = eis;  enabled * other = eis
BZK_HD uint32_t f_assert_eq_if(const Op& op, const TxView& v, const Arrays& A) {
    const Fr en = operand(v, op.in[0]), x = operand(v, op.in[1]), y = operand(v, op.in[2]);
    const bool on = !en.is_zero();
    const Fr ev = on ? x : Fr::zero();
    const size_t a = v.aux_base + op.aux_off, c = v.con_base + op.con_off;
    A.z_aux[a] = ev;
    A.az[c] = en; A.bz[c] = x; A.cz[c] = ev;
    A.az[c + 1] = en; A.bz[c + 1] = y; A.cz[c + 1] = ev;
    return on && !x.equals(y) ? FLAG_UNSATISFIED : 0u;
}
// this * 1 = other
BZK_HD uint32_t f_enforce_eq(const Op& op, const TxView& v, const Arrays& A) {
    const Fr x = operand(v, op.in[0]), y = operand(v, op.in[1]);
    const size_t c = v.con_base + op.con_off;
    A.az[c] = x; A.bz[c] = fr_one_mont(); A.cz[c] = y;
    return x.equals(y) ? 0u : FLAG_UNSATISFIED;
}
// no slot: the state a transition computes against the state the witness builder predicted for it
BZK_HD uint32_t f_check_eq(const Op& op, const TxView& v) { return operand(v, op.in[0]).equals(operand(v, op.in[1])) ? 0u : FLAG_CHAIN; }

// ---- the EdDSA gadget's ladders (Defer::sig; /root/reference/src/zk/groth16/gadgets/eddsa/mod.rs:77-280, host form host_r1cs.h APoint) -----------
// V_LADDER / F_LADDER, one pair per double-and-add ladder.  t = 0: the variable base (pk.mul(h)) followed by the signature's tail (+ sig_r, the three
// doublings of mul_cofactor), t = 1: the fixed base (g_base_mul(s)).  Operands (inputs): in[0], in[1] the base, in[2] the scalar (its strict
// decomposition stays on the host, the bits are read off its value), in[3] Jubjub's d, in[4], in[5] sig_r (t = 0).  `out`: the first of
// ladder_regs(t) registers, on both ops (F_LADDER reads what V_LADDER wrote):
//   point k at out + 2k (x, y): step s (0 .. 253) doubles into point 2s and adds the base into point 2s + 1; the tail's four sums are points 508 ..;
//   the ladder's result (the last step's mux) at out + 2 ladder_points(t); then one scratch register per point (pass 1's batch inversion)
// Slots (contiguous from aux_off / con_off): per step add(R, R) 9, add(D, base) 9 (t = 0) or add_const(D, base) 3 (t = 1), the two muxes 1 + 1;
// then (t = 0) the tail's four additions, 9 each.
constexpr uint32_t LADDER_STEPS = 254;  // a strict decomposition has 255 bits; the host muxes the first
BZK_HD uint32_t ladder_step_slots(int t) { return t == 0 ? 20u : 14u; }
BZK_HD uint32_t ladder_points(int t) { return 2u * LADDER_STEPS + (t == 0 ? 4u : 0u); }
BZK_HD uint32_t ladder_regs(int t) { return 3u * ladder_points(t) + 2u; }
BZK_HD uint32_t ladder_slots(int t) { return LADDER_STEPS * ladder_step_slots(t) + (t == 0 ? 4u * 9u : 0u); }
BZK_HD uint32_t ladder_lanes(int t) { return LADDER_STEPS + (t == 0 ? 4u : 0u); }  // pass 2: one lane per step / tail addition
// the value of the register a ladder names as its result: t = 0 the tail's last point, t = 1 the ladder's own result
BZK_HD uint32_t ladder_result_reg(int t) { return t == 0 ? 2u * (2u * LADDER_STEPS + 3u) : 2u * ladder_points(t); }

// selections limb by limb: a select between two aggregates becomes a private copy (scratch or LDS) on the device
BZK_HD Fr fr_sel(bool c, const Fr& a, const Fr& b) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
// the pass-2 products: one resident copy of the 8 x 32-bit product, called (inlined at every site the fill kernel held 350+ registers)
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t wf_u32x4 __attribute__((ext_vector_type(4)));
__device__ __noinline__ static Fr fr_mul_call(wf_u32x4 a0, wf_u32x4 a1, wf_u32x4 b0, wf_u32x4 b1) {
    Fr a, b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a.l[i] = a0[i]; a.l[4 + i] = a1[i];
        b.l[i] = b0[i]; b.l[4 + i] = b1[i];
    }
    return fe_mul<FrParams>(a, b);
}
BZK_HD Fr fr_mul(const Fr& a, const Fr& b) {
    return fr_mul_call(wf_u32x4{a.l[0], a.l[1], a.l[2], a.l[3]}, wf_u32x4{a.l[4], a.l[5], a.l[6], a.l[7]}, wf_u32x4{b.l[0], b.l[1], b.l[2], b.l[3]},
                       wf_u32x4{b.l[4], b.l[5], b.l[6], b.l[7]});
}
#else
BZK_HD Fr fr_mul(const Fr& a, const Fr& b) { return fe_mul<FrParams>(a, b); }
#endif

// bit j (most significant first) of the strict 255-bit decomposition of a canonical scalar
BZK_HD bool ladder_bit(const Fr& canon, uint32_t j) {
    const uint32_t i = 254u - j, w = i >> 5;
    uint32_t x = canon.l[0];
#pragma unroll
    for (uint32_t k = 1; k < 8; ++k) x = w == k ? canon.l[k] : x;  // no run-time index into the limbs (it would put them in LDS / scratch)
    return (x >> (i & 31u)) & 1u;
}
// PointAffine::is_on_curve (a = -1): y^2 - x^2 == 1 + d x^2 y^2
BZK_HD bool jj_on_curve(const Fr& x, const Fr& y, const Fr& d) {
    const Fr xx = fr_mul(x, x), yy = fr_mul(y, y);
    return fe_sub<FrParams>(yy, xx).equals(fe_add<FrParams>(Fr::one(), fr_mul(d, fr_mul(xx, yy))));
}
// projective Jubjub on the 29-bit form (x = X / Z, y = Y / Z; the unified formulas are complete on the curve: d is a non-square)
struct JP {
    Fr29 X, Y, Z;
};
BZK_HD JP jp_sel(bool c, const JP& a, const JP& b) {
    JP r;
#pragma unroll
    for (int i = 0; i < fr29::N; ++i) {
        r.X.l[i] = c ? a.X.l[i] : b.X.l[i];
        r.Y.l[i] = c ? a.Y.l[i] : b.Y.l[i];
        r.Z.l[i] = c ? a.Z.l[i] : b.Z.l[i];
    }
    return r;
}
BZK_HD JP jp_dbl(const JP& p) {  // dbl-2008-bbjlp with a = -1 (host_zk.hip Proj::dbl); k bounds in the comments (products need ka kb <= 70)
    const Fr29 xy2 = fr29::mul(fr29::add(p.X, p.X), p.Y);              // 2 X Y
    const Fr29 c = fr29::sqr(p.X), d = fr29::sqr(p.Y);
    const Fr29 f = fr29::sub3(d, c);                                   // Y^2 - X^2           k 5
    const Fr29 j = fr29::sub3(f, fr29::mul(fr29::add(p.Z, p.Z), p.Z)); // f - 2 Z^2           k 8
    const Fr29 m = fr29::sub3(fr29::sub3(fr29::zero(), c), d);         // -X^2 - Y^2          k 6
    return {fr29::mul(xy2, j), fr29::mul(f, m), fr29::mul(f, j)};
}
BZK_HD JP jp_add_affine(const JP& p, const Fr29& x2, const Fr29& y2, const Fr29& dc) {  // add-2008-bbjlp, Z2 = 1, a = -1 (host_zk.hip Proj::add_assign)
    const Fr29 b = fr29::sqr(p.Z);
    const Fr29 c = fr29::mul(p.X, x2), d = fr29::mul(p.Y, y2);
    const Fr29 e = fr29::mul(fr29::mul(dc, c), d);
    const Fr29 f = fr29::sub3(b, e);                                   // k 5
    const Fr29 g = fr29::norm(fr29::add(b, e));                        // k 4
    const Fr29 u = fr29::sub3(fr29::sub3(fr29::mul(fr29::add(p.X, p.Y), fr29::add(x2, y2)), c), d);  // X y2 + Y x2   k 8
    return {fr29::mul(fr29::mul(p.Z, f), u), fr29::mul(fr29::mul(p.Z, g), fr29::add(d, c)), fr29::mul(f, g)};
}

// pass 1: every point of one ladder (and its tail), affine, with ONE inversion (Montgomery's trick).  Each sum is the native one only where both of its
// operands are on the curve, (0, 0) otherwise - decided per addition, as the gadget does (an off-curve base still doubles the identity to the identity).
// Forward: point k is stored as (X pre_k, Y pre_k) with pre_k the product of the Z before it, its Z in the scratch register; backward: one product
// by the running inverse each (fr29::from29_scaled folds the conversion to the memory form into it).
BZK_HD void v_ladder(const Op& op, const TxView& v) {
    const int t = op.t;
    const Fr bxF = operand(v, op.in[0]), byF = operand(v, op.in[1]), dF = operand(v, op.in[3]);
    const Fr sc = fe_from_mont<FrParams>(operand(v, op.in[2]));
    const uint32_t np = ladder_points(t), zreg = 2u * np + 2u;
    Fr* const regs = v.regs + (size_t)op.out * v.reg_stride;
    const size_t rs = v.reg_stride;
    const bool base_on = jj_on_curve(bxF, byF, dF);
    const Fr29 bx = fr29::to29(bxF), by = fr29::to29(byF), dc = fr29::to29(dF), one = fr29::from_consts(fr29::ONE), zero = fr29::zero();
    const JP ZERO = {zero, zero, one}, IDENT = {zero, one, one};
    Fr29 acc = one;
    auto push = [&](uint32_t k, const JP& p) {
        regs[(size_t)(2u * k) * rs] = fr29::repack_to32(fr29::mul(p.X, acc));
        regs[(size_t)(2u * k + 1u) * rs] = fr29::repack_to32(fr29::mul(p.Y, acc));
        regs[(size_t)(zreg + k) * rs] = fr29::repack_to32(p.Z);
        acc = fr29::mul(acc, p.Z);
    };
    const bool b0 = ladder_bit(sc, 0);
    JP r = jp_sel(b0, JP{bx, by, one}, IDENT);
    bool r_on = b0 ? base_on : true;
#pragma unroll 1
    for (uint32_t s = 0; s < LADDER_STEPS; ++s) {
        const JP d2 = jp_dbl(r);
        const JP a2 = jp_add_affine(d2, bx, by, dc);
        const JP D = jp_sel(r_on, d2, ZERO), A = jp_sel(r_on && base_on, a2, ZERO);
        push(2u * s, D);
        push(2u * s + 1u, A);
        const bool bit = ladder_bit(sc, s + 1u);
        r = jp_sel(bit, A, D);
        r_on = bit ? (r_on && base_on) : r_on;
    }
    if (t == 0) {  // + sig_r, then mul_cofactor's three doublings
        const Fr rxF = operand(v, op.in[4]), ryF = operand(v, op.in[5]);
        const bool s_on = r_on && jj_on_curve(rxF, ryF, dF);
        JP q = jp_add_affine(r, fr29::to29(rxF), fr29::to29(ryF), dc);
#pragma unroll 1
        for (uint32_t j = 0; j < 4u; ++j) {
            if (j) q = jp_dbl(q);
            push(2u * LADDER_STEPS + j, jp_sel(s_on, q, ZERO));
        }
    }
    // acc = the product of every Z (none is zero: the formulas are complete on the curve, off-curve points are (0 : 0 : 1)); s = its inverse * 2^256
    Fr29 s = fr29::mul(fr29::inv(acc), fr29::from_consts(fr29::C_OUT));
#pragma unroll 1
    for (uint32_t k = np; k-- > 0;) {
        const Fr29 X = fr29::repack_from32(regs[(size_t)(2u * k) * rs]), Y = fr29::repack_from32(regs[(size_t)(2u * k + 1u) * rs]);
        const Fr29 Z = fr29::repack_from32(regs[(size_t)(zreg + k) * rs]);
        regs[(size_t)(2u * k) * rs] = fr29::from29_scaled(X, s);
        regs[(size_t)(2u * k + 1u) * rs] = fr29::from29_scaled(Y, s);
        s = fr29::mul(s, Z);
    }
    const uint32_t last = 2u * (2u * (LADDER_STEPS - 1u) + (ladder_bit(sc, LADDER_STEPS) ? 1u : 0u));
    regs[(size_t)(2u * np) * rs] = regs[(size_t)last * rs];
    regs[(size_t)(2u * np + 1u) * rs] = regs[(size_t)(last + 1u) * rs];
}

// pass 2: the slots of one addition, as APoint::add forms them.  Variables: sum x, y | x ox, (x ox) y, common = (x ox y) oy | x oy, y ox | y oy, x ox;
// constraints: the six products in allocation order around the two `enforce` rows (1 + d common) sum.x = x1 + x2, (1 - d common) sum.y = y1 + y2
BZK_HD void ladder_add_slots(const Arrays& A, size_t a, size_t c, const Fr& px, const Fr& py, const Fr& qx, const Fr& qy, const Fr& sx, const Fr& sy,
                             const Fr& d) {
    const Fr t1 = fr_mul(px, qx), t2 = fr_mul(t1, py), common = fr_mul(t2, qy);
    const Fr x1 = fr_mul(px, qy), x2 = fr_mul(py, qx), y1 = fr_mul(py, qy), y2 = fr_mul(px, qx);
    const Fr kd = fr_mul(d, common), one = Fr::one();
    A.z_aux[a] = sx; A.z_aux[a + 1] = sy; A.z_aux[a + 2] = t1; A.z_aux[a + 3] = t2; A.z_aux[a + 4] = common;
    A.z_aux[a + 5] = x1; A.z_aux[a + 6] = x2; A.z_aux[a + 7] = y1; A.z_aux[a + 8] = y2;
    A.az[c] = px; A.bz[c] = qx; A.cz[c] = t1;
    A.az[c + 1] = t1; A.bz[c + 1] = py; A.cz[c + 1] = t2;
    A.az[c + 2] = t2; A.bz[c + 2] = qy; A.cz[c + 2] = common;
    A.az[c + 3] = px; A.bz[c + 3] = qy; A.cz[c + 3] = x1;
    A.az[c + 4] = py; A.bz[c + 4] = qx; A.cz[c + 4] = x2;
    A.az[c + 5] = fe_add<FrParams>(one, kd); A.bz[c + 5] = sx; A.cz[c + 5] = fe_add<FrParams>(x1, x2);
    A.az[c + 6] = py; A.bz[c + 6] = qy; A.cz[c + 6] = y1;
    A.az[c + 7] = px; A.bz[c + 7] = qx; A.cz[c + 7] = y2;
    A.az[c + 8] = fe_sub<FrParams>(one, kd); A.bz[c + 8] = sy; A.cz[c + 8] = fe_add<FrParams>(y1, y2);
}
// lane `s` of an F_LADDER op: step s (< LADDER_STEPS) or, t = 0, the tail's addition s - LADDER_STEPS
BZK_HD void f_ladder(const Op& op, const TxView& v, const Arrays& A, uint32_t s) {
    const int t = op.t;
    const Fr* const regs = v.regs + (size_t)op.out * v.reg_stride;
    const size_t rs = v.reg_stride;
    const Fr d = operand(v, op.in[3]), one = Fr::one();
    const uint32_t ss = ladder_step_slots(t);
    if (s < LADDER_STEPS) {
        const Fr bx = operand(v, op.in[0]), by = operand(v, op.in[1]);
        const Fr sc = fe_from_mont<FrParams>(operand(v, op.in[2]));
        Fr px, py;  // the point entering the step: the host's first-bit muxes, or the previous step's mux
        if (s == 0) {
            const bool b0 = ladder_bit(sc, 0);
            px = fr_sel(b0, bx, Fr::zero());
            py = fr_sel(b0, by, one);
        } else {
            const uint32_t k = 2u * (2u * (s - 1u) + (ladder_bit(sc, s) ? 1u : 0u));
            px = regs[(size_t)k * rs];
            py = regs[(size_t)(k + 1u) * rs];
        }
        const Fr dx = regs[(size_t)(4u * s) * rs], dy = regs[(size_t)(4u * s + 1u) * rs], ax = regs[(size_t)(4u * s + 2u) * rs], ay = regs[(size_t)(4u * s + 3u) * rs];
        size_t a = v.aux_base + op.aux_off + (size_t)s * ss, c = v.con_base + op.con_off + (size_t)s * ss;
        ladder_add_slots(A, a, c, px, py, px, py, dx, dy, d);
        a += 9; c += 9;
        if (t == 0) {
            ladder_add_slots(A, a, c, dx, dy, bx, by, ax, ay, d);
            a += 9; c += 9;
        } else {  // add_const: sum x, y | common = x y;  x y = common, (1 + dbb common) sum.x = x by + y bx, (1 - dbb common) sum.y = y by + x bx
            const Fr dbb = fr_mul(fr_mul(d, bx), by), common = fr_mul(dx, dy), kx = fr_mul(dbb, common);
            A.z_aux[a] = ax; A.z_aux[a + 1] = ay; A.z_aux[a + 2] = common;
            A.az[c] = dx; A.bz[c] = dy; A.cz[c] = common;
            A.az[c + 1] = fe_add<FrParams>(one, kx); A.bz[c + 1] = ax; A.cz[c + 1] = fe_add<FrParams>(fr_mul(dx, by), fr_mul(dy, bx));
            A.az[c + 2] = fe_sub<FrParams>(one, kx); A.bz[c + 2] = ay; A.cz[c + 2] = fe_add<FrParams>(fr_mul(dy, by), fr_mul(dx, bx));
            a += 3; c += 3;
        }
        // mux(bit, D, A) for x and y:  ret = bit ? A : D,  (D - A) bit = D - ret
        const bool bit = ladder_bit(sc, s + 1u);
        const Fr rx = fr_sel(bit, ax, dx), ry = fr_sel(bit, ay, dy), bv = fr_sel(bit, one, Fr::zero());
        A.z_aux[a] = rx; A.az[c] = fe_sub<FrParams>(dx, ax); A.bz[c] = bv; A.cz[c] = fe_sub<FrParams>(dx, rx);
        A.z_aux[a + 1] = ry; A.az[c + 1] = fe_sub<FrParams>(dy, ay); A.bz[c + 1] = bv; A.cz[c + 1] = fe_sub<FrParams>(dy, ry);
        return;
    }
    if (t != 0 || s >= ladder_lanes(t)) return;
    const uint32_t j = s - LADDER_STEPS, sk = 2u * (2u * LADDER_STEPS + j);
    const uint32_t pk = j == 0 ? 2u * ladder_points(t) : sk - 2u;  // the ladder's result + sig_r, then each tail point doubled
    const Fr px = regs[(size_t)pk * rs], py = regs[(size_t)(pk + 1u) * rs];
    const Fr qx = fr_sel(j == 0, operand(v, op.in[4]), px), qy = fr_sel(j == 0, operand(v, op.in[5]), py);
    const size_t a = v.aux_base + op.aux_off + (size_t)LADDER_STEPS * ss + 9u * j, c = v.con_base + op.con_off + (size_t)LADDER_STEPS * ss + 9u * j;
    ladder_add_slots(A, a, c, px, py, qx, qy, regs[(size_t)sk * rs], regs[(size_t)(sk + 1u) * rs], d);
}

}  // namespace wf
}  // namespace bzk
