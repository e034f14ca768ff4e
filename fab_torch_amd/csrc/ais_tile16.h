// What the two 16-chain units share (ais_tile16.hip, ais_tile16_metropolis.hip): the per-tile state behind the flow's LDS plan,
// its two loaders and the LDS plan of a launch.  Include it behind ais_device.h.
#pragma once
#include "flow_device.h"
#include "defensive_device.h"

namespace fab {

struct ExtraLds {   // per-tile HMC state appended after the flow's LDS plan (floats)
    int o_XP, o_P, o_GU, o_GP, o_ROW, total;
};
static inline ExtraLds make_extra_lds(const FlowLds& l, int D) {
    ExtraLds e;
    int o = l.total;
    e.o_XP = o; o += ROWS * D;
    e.o_P = o; o += ROWS * D;
    e.o_GU = o; o += ROWS * D;
    e.o_GP = o; o += ROWS * D;
    e.o_ROW = o; o += 2 * ROWS;
    e.total = (o + 3) & ~3;
    return e;
}

__device__ __forceinline__ void load_state_to_u0(const FlowLds& l, int D, float* lds, const float* XP, const Tid& t) {
    for (int e = t.tid; e < ROWS * l.DS; e += NTHREADS) {
        const int r = e / l.DS, j = e % l.DS;
        lds[l.o_U0 + e] = j < D ? XP[r * D + j] : 0.f;
    }
}

__device__ __forceinline__ void zero_dp(const FlowLds& l, float* lds, const Tid& t) {
    for (int e = t.tid; e < ROWS * l.PS; e += NTHREADS) lds[l.o_DP + e] = 0.f;
}

// LDS of a 16-chain launch; `mx.on` (defensive mixture): the staged mixture parameters behind the kernel's plan
struct Lds16 {
    FlowLds l;
    ExtraLds x;
    size_t bytes;
};
static Lds16 make_lds16(const FlowDims& f, bool grad, const MixDev& mx) {
    Lds16 p;
    p.l = make_flow_lds(f, grad);
    p.x = make_extra_lds(p.l, f.D);
    p.bytes = (size_t)(p.x.total + (mx.on ? mix_lds_floats(f.D) : 0)) * 4;
    return p;
}

}  // namespace fab
