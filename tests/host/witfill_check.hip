// CPU harness of the signature-ladder device code (bazuka_amd/csrc/bzk_witfill.cuh V_LADDER, bzk_fr29.cuh inv): the same __host__ __device__
// functions the gfx950 kernels run, called from tests/test_defer_sig_cpu.py through ctypes.  All scalars are 32-byte Montgomery-256 limbs (ZkScalar).
#include <string.h>

#include <vector>

#include "../../bazuka_amd/csrc/bzk_witfill.cuh"

using namespace bzk;

extern "C" {

// out = in^-1 (0 for 0) through the 29-bit form
int hc_fr29_inv(const uint8_t in[32], uint8_t out[32]) {
    Fr a;
    memcpy(a.l, in, 32);
    const Fr r = fr29::from29(fr29::inv(fr29::to29(a)));
    memcpy(out, r.l, 32);
    return 0;
}

// one V_LADDER op (t = 0 variable base with the tail, t = 1 fixed base) on a single transition: points = ladder_points(t) affine points (x | y, 64 bytes
// each) followed by the result (64 bytes).  in = base x | base y | scalar | d | sig_r x | sig_r y.  Returns the number of points.
int hc_ladder(int t, const uint8_t in[6 * 32], uint8_t* out) {
    std::vector<Fr> inputs(6), regs(wf::ladder_regs(t));
    for (int i = 0; i < 6; ++i) memcpy(inputs[i].l, in + 32 * i, 32);
    wf::Op op{};
    op.kind = wf::V_LADDER;
    op.t = (uint8_t)t;
    op.out = 0;
    for (int i = 0; i < 6; ++i) op.in[i] = ~i;
    const wf::TxView v{inputs.data(), regs.data(), 1, 0, 0, nullptr};
    wf::v_ladder(op, v);
    const uint32_t np = wf::ladder_points(t);
    memcpy(out, regs.data(), (size_t)(2 * np + 2) * 32);
    return (int)np;
}
}
