// Defensive-mixture base distribution on the 16-chain tile of a workgroup
// (fab/trainable_distributions/defensive_mixture.py): log q = logsumexp(log q_flow + logsigmoid(l),
// log N(x; loc, exp(log_scale)) + logsigmoid(-l)), applied as an epilogue of flow_log_prob_tile - element-wise
// work on the tile, the shape of target_tile (target_device.h).  Definition: tests/defensive_spec.py.
#pragma once
#include "flow_device.h"
#include "target_device.h"

#pragma clang fp contract(off)   // a*b+c stays two roundings, like the eager reference

namespace fab {

// The kernels read the module's three parameter tensors themselves: no packed copy that could go stale, no host
// read of the logit.
struct MixDev {
    const float* loc;        // [D]
    const float* log_scale;  // [D]
    const float* logit;      // [1]
    int on;
};

static inline MixDev make_mix_dev(const fabhip_defensive_args* m) {
    if (!m || !m->enabled) return MixDev{nullptr, nullptr, nullptr, 0};
    return MixDev{m->loc, m->log_scale, m->logit, 1};
}

static inline int check_mix(const fabhip_defensive_args* m) {
    if (!m || !m->enabled) return FABHIP_OK;
    return (m->loc && m->log_scale && m->logit) ? FABHIP_OK : FABHIP_EINVAL;
}

// log sigmoid(l) = min(l, 0) - log1p(exp(-|l|))
__device__ __forceinline__ float mix_logsigmoid(float l) { return fminf(l, 0.f) - log1pf(expf(-fabsf(l))); }
// P(flow branch) = sigmoid(l), the two-sided form (no overflow for l << 0)
__device__ __forceinline__ float mix_sigmoid(float l) {
    const float e = expf(-fabsf(l));
    return l >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// The kernels stage the parameters in LDS once per launch, behind the kernel's own plan (4 D + 4 floats):
//   loc [D] | log_scale [D] | exp(-log_scale) [D] | exp(-2 log_scale) [D] | logsigmoid(l), logsigmoid(-l), sigmoid(l)
// The epilogue then needs no global pointer and no constant of the log1p expansion, whose registers would otherwise stay
// allocated across the flow's register-resident weight stages (hipcc hoists them out of the leapfrog loop), and a leapfrog
// re-reads a few LDS words instead of memory.  A barrier of the caller separates mix_stage from the first mix_tile.
static inline int mix_lds_floats(int D) { return 4 * D + 4; }
__device__ __forceinline__ void mix_stage(const MixDev& mx, int D, float* MP, const Tid& t) {
    for (int e = t.tid; e < D; e += NTHREADS) {
        const float ls = mx.log_scale[e];
        MP[e] = mx.loc[e]; MP[D + e] = ls; MP[2 * D + e] = expf(-ls); MP[3 * D + e] = expf(-2.f * ls);
    }
    if (t.tid == 0) {
        const float l = mx.logit[0];
        MP[4 * D] = mix_logsigmoid(l); MP[4 * D + 1] = mix_logsigmoid(-l); MP[4 * D + 2] = mix_sigmoid(l);
    }
}

// MP: the staged parameters.  XP: LDS [16][ldx] positions; G: LDS [16][ldg] holds d log q_flow / dx on entry and d log q / dx on return (GRAD).
// Each thread touches the (row, j = c, c + 16, ...) elements only - the mapping of every reader that follows - so no
// barrier is needed around the call.  Returns the mixture log q of this thread's row (replicated over its 16 lanes).
template <bool GRAD>
__device__ float mix_tile(const float* MP, int D, const float* XP, int ldx, float* G, int ldg, float lq_flow, const Tid& t) {
    float acc = 0.f;
    for (int j = t.c; j < D; j += 16) {
        const float z = (XP[t.row * ldx + j] - MP[j]) * MP[2 * D + j];
        acc += -0.5f * (z * z) - MP[D + j];
    }
    const float a = lq_flow + MP[4 * D];
    const float b = (row16_sum(acc) - 0.5f * (float)D * 1.8378770664093453f) + MP[4 * D + 1];
    const float m = fmaxf(a, b);
    float lq;
    if (a != a || b != b) lq = NAN;
    else if (m == -INFINITY) lq = -INFINITY;                    // (no (-inf) - (-inf))
    else lq = m + logf(expf(a - m) + expf(b - m));
    if (GRAD) {
        // responsibility of the flow; exactly 0 where a = -inf, and the flow's gradient then contributes 0 whatever it holds
        const float rf = (a == -INFINITY) ? 0.f : expf(a - lq);
        for (int j = t.c; j < D; j += 16) {
            const float gn = -(XP[t.row * ldx + j] - MP[j]) * MP[3 * D + j];
            const float gf = (rf == 0.f) ? 0.f : rf * G[t.row * ldg + j];
            G[t.row * ldg + j] = gf + (1.f - rf) * gn;
        }
    }
    return lq;
}

}  // namespace fab
