// The batched verifier's per-proof functions (bazuka_amd/csrc/bzk_pairing28.cuh) in their DEVICE-field instantiation (Fp28Ops / Fp2x28Ops on the
// slots of a strided Lane28 slab), run on the CPU with the bound assertions of bzk_fp28.cuh on, against the 64-bit-limb host instantiation (hp::)
// as canonical values.  A stand-alone program: prints one line per check, exits 0 when all hold (an assertion aborts).
// What this shows and what it does not: hp:: is the SAME template text over the other field, so agreement here says that the two fields agree,
// that no operand leaves the bounds of bzk_fp28.cuh and that the strided lane addresses its slots as the flat one does.  It cannot catch a wrong
// formula or aliased slots shared by both instantiations: that rests on tests/test_pairing_cpu.py and tests/host/hostcheck.hip, which compare
// hp:: with independent, slower forms (the affine loop, the plain exponentiation, the Python reference).
#define BZK_FP28_CHECK 1
#include <stdio.h>

#include <vector>

#include "../../bazuka_amd/csrc/host_pairing.h"

using namespace bzk;
using pairing::Lane28;
namespace sl = pairing::slot;
typedef pairing::Tower<Fp28Ops, Fp2x28Ops> TW28;

static int g_bad = 0;
static void check(bool ok, const char* what) {
    printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++g_bad;
}

static uint64_t rng(uint64_t& st) { st += 0x9e3779b97f4a7c15ull; uint64_t z = st; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
static HFp rand_fp(uint64_t& st) {
    HFp a;
    for (int i = 0; i < 6; ++i) a.l[i] = rng(st);
    a.l[5] &= 0x0fffffffffffffffull;  // < 2^380 < p
    return a;
}
static HFp2 rand_fp2(uint64_t& st) { return {rand_fp(st), rand_fp(st)}; }
// the edge operands: 0, 1, p - 1 (as Montgomery values), else random
static HFp edge_fp(uint64_t& st, int kind) {
    if (kind == 0) return HFpOps::zero();
    if (kind == 1) return HFpOps::one();
    if (kind == 2) return HFpOps::neg(HFpOps::one());
    return rand_fp(st);
}
static hp::E12 rand_e12(uint64_t& st, int edge) {   // edge: some coefficients from the edge set
    hp::E12 f;
    HFp* v = (HFp*)&f;
    for (int i = 0; i < 12; ++i) v[i] = edge ? edge_fp(st, (int)(rng(st) % 5)) : rand_fp(st);
    return f;
}
static Fp28 to28h(const HFp& a) { return hp::h_to28(a); }
static HFp from28h(const Fp28& a) {
    const Fp t = fp28::from28(a);
    HFp r;
    memcpy(r.l, t.l, 48);
    return r;
}
static Fp2x28 to28h(const HFp2& a) { return {to28h(a.c0), to28h(a.c1)}; }
static HFp2 from28h(const Fp2x28& a) { return {from28h(a.c0), from28h(a.c1)}; }

// a slab of `lanes` proofs as the kernels lay it out; the checks run lane `lane` of it
struct Slab {
    std::vector<uint32_t> w;
    uint32_t stride;
    Lane28 l;
    Slab(uint32_t lanes, uint32_t lane) : w((size_t)sl::COUNT * 14 * lanes, 0xdeadbeefu), stride(lanes), l{w.data() + lane, lanes} {}
    void put12(int at, const hp::E12& a) { for (int i = 0; i < 12; ++i) l.st1(at + i, to28h(((const HFp*)&a)[i])); }
    hp::E12 get12(int at) const { hp::E12 r; for (int i = 0; i < 12; ++i) ((HFp*)&r)[i] = from28h(l.ld1(at + i)); return r; }
    void put2(int at, const HFp2& a) { pairing::st2(l, at, to28h(a)); }
    void put1(int at, const HFp& a) { l.st1(at, to28h(a)); }
};

static HFp fp_pow(const HFp& a, const uint64_t* e, int limbs) {
    HFp r = HFpOps::one();
    for (int i = 64 * limbs - 1; i >= 0; --i) {
        r = HFpOps::sqr(r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = HFpOps::mul(r, a);
    }
    return r;
}
// a point of y^2 = x^3 + 4 from a seed (p = 3 mod 4: a square root is a^((p + 1) / 4))
static hp::G1A curve_point(uint64_t& st) {
    uint64_t e[6];
    memcpy(e, hfp::consts().p, 48);
    e[0] += 1;   // p + 1 (no carry: the low limb of p is not all ones)
    for (int i = 0; i < 6; ++i) e[i] = (e[i] >> 2) | (i < 5 ? e[i + 1] << 62 : 0);
    for (;;) {
        const HFp x = rand_fp(st);
        const HFp rhs = HFpOps::add(HFpOps::mul(HFpOps::sqr(x), x), hp::fp_four());
        const HFp y = fp_pow(rhs, e, 6);
        if (HFpOps::eq(HFpOps::sqr(y), rhs)) return {x, y, false};
    }
}
static void pack_g1(uint8_t* out, const hp::G1A& p) {
    memcpy(out, p.x.l, 48); memcpy(out + 48, p.y.l, 48);
    out[96] = p.inf ? 1 : 0;
}

int main() {
    uint64_t st = 0x42415a554b41ull;
    // ---- the tower, piece by piece: random operands, edge operands, outputs of earlier products
    for (int round = 0; round < 6; ++round) {
        const int edge = round >= 3;
        hp::E12 f = rand_e12(st, edge), g = rand_e12(st, edge);
        if (round == 2 || round == 5) { f = hp::e12_mul(f, g); g = hp::e12_sqr(g); }   // outputs of earlier products
        Slab S(3, round % 3);
        {
            TW28::E6 a = {to28h(f.a0.c0), to28h(f.a0.c1), to28h(f.a0.c2)}, b = {to28h(g.a1.c0), to28h(g.a1.c1), to28h(g.a1.c2)};
            const TW28::E6 r = TW28::e6_mul(a, b);
            const hp::E6 want = hp::e6_mul(f.a0, g.a1), got = {from28h(r.c0), from28h(r.c1), from28h(r.c2)};
            check(hp::e6_eq(got, want), "e6_mul");
            const TW28::E6 r2 = TW28::e6_mul(r, r);   // operands that are product outputs
            const hp::E6 got2 = {from28h(r2.c0), from28h(r2.c1), from28h(r2.c2)};
            check(hp::e6_eq(got2, hp::e6_mul(want, want)), "e6_mul of products");
        }
        S.put12(sl::F, f); S.put12(sl::R1, g);
        pairing::e12_mul(S.l, sl::R2, sl::F, sl::R1, sl::TMP);
        check(hp::e12_eq(S.get12(sl::R2), hp::e12_mul(f, g)), "e12_mul");
        pairing::e12_mul(S.l, sl::R2, sl::R2, sl::R2, sl::TMP);   // in place, operands = an earlier product
        check(hp::e12_eq(S.get12(sl::R2), hp::e12_sqr(hp::e12_mul(f, g))), "e12_mul in place");
        pairing::e12_sqr(S.l, sl::R3, sl::F, sl::TMP);
        check(hp::e12_eq(S.get12(sl::R3), hp::e12_sqr(f)), "e12_sqr");
        {
            const HFp2 c0 = {edge_fp(st, edge ? 2 : 3), rand_fp(st)}, c1 = rand_fp2(st), c4 = {rand_fp(st), edge_fp(st, edge ? 0 : 3)};
            S.put12(sl::R3, f);
            S.put2(sl::LINE, c0); S.put2(sl::LINE + 2, c1); S.put2(sl::LINE + 4, c4);
            pairing::e12_mul_by_014(S.l, sl::R3, sl::LINE, sl::TMP);
            check(hp::e12_eq(S.get12(sl::R3), hp::e12_mul_by_014(f, c0, c1, c4)), "e12_mul_by_014");
        }
        if (!hp::e12_eq(f, hp::E12{hp::e6_zero(), hp::e6_zero()})) {
            pairing::e12_inv(S.l, sl::R3, sl::F, sl::TMP);
            check(hp::e12_eq(S.get12(sl::R3), hp::e12_inv(f)), "e12_inv");
        }
        std::vector<Fp2x28> frob(6);
        for (int i = 0; i < 6; ++i) frob[i] = to28h(hp::frob_consts().g[i]);
        pairing::e12_frob(S.l, sl::R3, sl::F, frob.data());
        check(hp::e12_eq(S.get12(sl::R3), hp::e12_frob(f)), "e12_frob");
        // the cyclotomic forms on an element of that subgroup: the easy part of the final exponentiation
        const hp::E12 m = hp::final_exp_easy(f);
        S.put12(sl::R1, m);
        pairing::e12_cyc_sqr(S.l, sl::R2, sl::R1);
        check(hp::e12_eq(S.get12(sl::R2), hp::e12_cyc_sqr(m)), "e12_cyc_sqr");
        if (round < 2 || round == 3) {
            pairing::e12_cyc_exp_x(S.l, sl::R2, sl::R1, sl::TMP);
            check(hp::e12_eq(S.get12(sl::R2), hp::e12_cyc_exp_x(m)), "e12_cyc_exp_x");
            S.put12(sl::F, f);
            pairing::final_exp(S.l, frob.data());
            check(hp::e12_eq(S.get12(sl::R4), hp::final_exp(f)), "final_exp");
        }
    }
    // ---- the table-driven Miller loop times m against the four-pair loop, on made-up points (the formulas are identities in the coordinates)
    for (int round = 0; round < 3; ++round) {
        hp::G1A ps[4];
        hp::G2A qs[4];
        for (int k = 0; k < 4; ++k) { ps[k] = {rand_fp(st), rand_fp(st), false}; qs[k] = {rand_fp2(st), rand_fp2(st), false}; }
        const uint32_t live = round == 0 ? 7u : round == 1 ? 5u : 6u;   // which of (A, B), (X, gamma), (C, delta) are live
        ps[0].inf = !(live & 1); ps[1].inf = !(live & 2); qs[2].inf = !(live & 4);
        bool deg = false;
        const hp::E12 want = hp::multi_miller(ps, qs, 4, &deg);
        hp::KeyHost K;
        K.n_inputs = 0;
        K.tab_xy.assign(2, HFpOps::zero()); K.tab_inf.assign(1, 1);
        K.gamma_live = 1; K.delta_live = !qs[2].inf;
        K.gamma_steps = hp::line_table(qs[1], K.gamma);
        K.delta_steps = qs[2].inf ? (uint32_t)pairing::MILLER_STEPS : hp::line_table(qs[2], K.delta);
        if (qs[2].inf) K.delta.assign((size_t)3 * pairing::MILLER_STEPS, HFp2Ops::zero());
        const hp::E12 m = hp::multi_miller(ps + 3, qs + 3, 1, &deg);
        memcpy(K.m, &m, sizeof m);
        const hp::KeyUpload up(K);
        const auto k28 = up.view(K, up.bytes.data());
        Slab S(5, 2);
        uint32_t flags = 0;
        if (!ps[0].inf) { flags |= pairing::FLAG_AB; S.put1(sl::PA, ps[0].x); S.put1(sl::PA + 1, ps[0].y); }
        S.put2(sl::QB, qs[0].x); S.put2(sl::QB + 2, qs[0].y);
        if (!ps[1].inf) { flags |= pairing::FLAG_X; S.put1(sl::PX, ps[1].x); S.put1(sl::PX + 1, ps[1].y); }
        flags |= pairing::FLAG_C; S.put1(sl::PC, ps[2].x); S.put1(sl::PC + 1, ps[2].y);
        const uint32_t out = pairing::miller_one(S.l, k28, flags);
        check(!deg && out == flags && K.gamma_steps == 68 && hp::e12_eq(S.get12(sl::F), want), "miller_one * m == four-pair multi_miller");
        // the host-field instantiation of the same function
        HFp hs[sl::COUNT];
        const hp::LaneH lh = {hs};
        hs[sl::PA] = ps[0].x; hs[sl::PA + 1] = ps[0].y; hs[sl::PX] = ps[1].x; hs[sl::PX + 1] = ps[1].y; hs[sl::PC] = ps[2].x; hs[sl::PC + 1] = ps[2].y;
        memcpy(hs + sl::QB, &qs[0].x, 96); memcpy(hs + sl::QB + 2, &qs[0].y, 96);
        check(pairing::miller_one(lh, K.view(), flags) == flags && hp::e12_eq(hp::get12(hs, sl::F), want), "miller_one over the host field");
    }
    // ---- both degenerate exits are reported, not computed
    {
        Slab S(2, 1);
        const HFp2 qx = rand_fp2(st), qy = rand_fp2(st);
        S.put1(sl::PA, rand_fp(st)); S.put1(sl::PA + 1, rand_fp(st));
        S.put2(sl::QB, qx); S.put2(sl::QB + 2, HFp2Ops::zero());   // a running point with Y = 0
        hp::KeyHost K;
        K.gamma.assign(3 * 68, HFp2Ops::zero()); K.delta = K.gamma;
        K.tab_xy.assign(2, HFpOps::zero()); K.tab_inf.assign(1, 1);
        K.gamma_steps = K.delta_steps = 68;
        const hp::E12 one = hp::e12_one();
        memcpy(K.m, &one, sizeof one);
        const hp::KeyUpload up(K);
        const auto k28 = up.view(K, up.bytes.data());
        check(pairing::miller_one(S.l, k28, pairing::FLAG_AB) == (pairing::FLAG_AB | pairing::FLAG_DEGENERATE), "Y = 0 is degenerate");
        for (int sign = 0; sign < 2; ++sign) {   // T = +-Q at an addition
            S.put2(sl::QB, qx); S.put2(sl::QB + 2, qy);
            S.put2(sl::TT, qx); S.put2(sl::TT + 2, sign ? HFp2Ops::neg(qy) : qy); S.put2(sl::TT + 4, HFp2Ops::one());
            check(!pairing::s_add_step(S.l, sl::TT, sl::QB, sl::PA, sl::LINE), sign ? "T = -Q is degenerate" : "T = Q is degenerate");
        }
        // a fixed argument whose table stops short: reported when its pair is live, ignored when it is not
        hp::G2A q0 = {qx, HFp2Ops::zero(), false};
        std::vector<HFp2> tab;
        check(hp::line_table(q0, tab) == 0, "line_table stops at Y = 0");
        K.gamma_steps = 0; K.gamma_live = 1;
        const auto k2 = hp::KeyUpload(K).view(K, up.bytes.data());
        S.put1(sl::PX, rand_fp(st)); S.put1(sl::PX + 1, rand_fp(st));
        check(pairing::miller_one(S.l, k2, pairing::FLAG_X) == (pairing::FLAG_X | pairing::FLAG_DEGENERATE), "degenerate gamma with X finite");
        check(pairing::miller_one(S.l, k2, 0) == 0 && hp::e12_is_one(S.get12(sl::F)), "degenerate gamma with X at infinity contributes 1");
    }
    // ---- prepare_one: X = IC_0 + sum x_i IC_i through the windows equals a plain double-and-add; checks of the proof's points
    {
        const uint32_t n_in = 3;
        std::vector<uint8_t> vk(878 + 97 * (n_in + 1), 0);
        vk[96] = 1; vk[194 + 192] = 1; vk[387 + 192] = 1; vk[677 + 192] = 1;   // alpha .. delta at infinity: this block is about IC only
        const uint64_t n_ic = n_in + 1;
        memcpy(vk.data() + 870, &n_ic, 8);
        std::vector<hp::G1A> ic(n_ic);
        for (auto& p : ic) p = curve_point(st);
        for (uint32_t i = 0; i < n_ic; ++i) pack_g1(vk.data() + 878 + 97 * i, ic[i]);
        hp::KeyHost K;
        hp::key_prepare(vk.data(), vk.size(), n_in, K);
        check(K.valid, "key_prepare accepts a key of curve points");
        const hp::KeyUpload up(K);
        const auto k28 = up.view(K, up.bytes.data());
        for (int round = 0; round < 4; ++round) {
            Fr x[3];
            for (auto& s : x) {
                for (int w = 0; w < 8; ++w) s.l[w] = (uint32_t)rng(st);
                s.l[7] &= 0x3fffffffu;   // canonical scalars below r
            }
            if (round == 1) { x[0] = Fr::zero(); x[1] = Fr::zero(); x[1].l[0] = 1; for (int w = 0; w < 8; ++w) x[2].l[w] = FrParams::MOD[w]; x[2].l[0] -= 1; }
            if (round == 2) for (int w = 0; w < 8; ++w) { x[0].l[w] = 0xffffffffu >> (w == 7 ? 4 : 0); x[1].l[w] = 0x88888888u >> (w == 7 ? 4 : 0); x[2].l[w] = 0; }
            uint8_t inputs[96], proof[387] = {0};
            for (int i = 0; i < 3; ++i) { const Fr mont = fe_to_mont<FrParams>(x[i]); memcpy(inputs + 32 * i, mont.l, 32); }
            proof[96] = proof[289] = proof[386] = 1;   // A, B, C at infinity: no point to check, X is computed all the same
            typedef XyzzT<HFpOps> Pt;
            Pt want = xyzz_from_affine<HFpOps>({ic[0].x, ic[0].y});
            for (int i = 0; i < 3; ++i) {
                Pt r = xyzz_identity<HFpOps>();
                const Pt b = xyzz_from_affine<HFpOps>({ic[i + 1].x, ic[i + 1].y});
                for (int bit = 255; bit >= 0; --bit) {
                    r = xyzz_dbl<HFpOps>(r);
                    if ((x[i].l[bit >> 5] >> (bit & 31)) & 1) xyzz_add<HFpOps>(r, b);
                }
                xyzz_add<HFpOps>(want, r);
            }
            AffineT<HFpOps> wa;
            const bool finite = xyzz_to_affine<HFpOps>(want, wa);
            Slab S(4, 3);
            uint32_t sc[24 * 4];   // word-major with the slab's stride, this lane's column
            const uint32_t flags = pairing::prepare_one(S.l, k28, inputs, proof, sc + 3, 4);
            check(finite && flags == pairing::FLAG_X && HFpOps::eq(from28h(S.l.ld1(sl::PX)), wa.x) && HFpOps::eq(from28h(S.l.ld1(sl::PX + 1)), wa.y),
                  "prepare_one: X equals double-and-add");
            if (round == 0) {
                // finite A and C on the curve are accepted and stored; one off it, limbs >= p, an input >= r are refused
                const hp::G1A a = curve_point(st);
                pack_g1(proof, a); pack_g1(proof + 290, a);
                const uint32_t f2 = pairing::prepare_one(S.l, k28, inputs, proof, sc + 3, 4);
                check(f2 == (pairing::FLAG_X | pairing::FLAG_C) && HFpOps::eq(from28h(S.l.ld1(sl::PA + 1)), a.y), "prepare_one: finite A, C");
                proof[0] ^= 1;
                check(pairing::prepare_one(S.l, k28, inputs, proof, sc + 3, 4) == pairing::FLAG_REFUSED, "prepare_one: A off the curve");
                memcpy(proof, hfp::consts().p, 48);
                check(pairing::prepare_one(S.l, k28, inputs, proof, sc + 3, 4) == pairing::FLAG_REFUSED, "prepare_one: limbs >= p");
                pack_g1(proof, a);
                memcpy(inputs + 32, FrParams::MOD, 32);
                check(pairing::prepare_one(S.l, k28, inputs, proof, sc + 3, 4) == pairing::FLAG_REFUSED, "prepare_one: input limbs >= r");
            }
        }
    }
    printf(g_bad ? "%d checks FAILED\n" : "all checks hold (%d failed)\n", g_bad);
    return g_bad ? 1 : 0;
}
