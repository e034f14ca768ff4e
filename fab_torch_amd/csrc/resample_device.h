// Device functions that more than one group of resampler kernels uses (resample_scan.hip, resample_emit.hip,
// weight_decisions.hip): the specified exponential and the fixed-point weight, 64-bit wave shuffles, the stratum map of the
// systematic / stratified resamplers and the hash of the seeded ones.  No kernel lives here.
#pragma once
#include "fabhip_common.h"

#pragma clang fp contract(off)

namespace fab {

// Specified fp32 exponential of the resampler (oracle/numerical.py:exp_spec restates it op for op):
//   r = x * log2(e); k = rint(r); f = r - k; p = 2^k * P6(f)   with every multiply and add individually rounded
// (no FMA contraction in a unit that includes this file), x <= 0.  Deterministic on any IEEE machine => bit-exact parity of the
// resulting fixed-point CDF; |p/exp(x) - 1| <= 2e-6 (3e-7 near the maximum).
__device__ __forceinline__ float exp_spec(float x) {
    const float r = x * 1.44269504088896341f;
    const float k = rintf(r);
    const float f = r - k;
    float p = 1.5403530393381609e-4f;
    p = p * f + 1.3333558146428443e-3f;
    p = p * f + 9.6181291076284772e-3f;
    p = p * f + 5.5504108664821580e-2f;
    p = p * f + 2.4022650695910071e-1f;
    p = p * f + 6.9314718055994531e-1f;
    p = p * f + 1.0f;
    return (k < -60.f) ? 0.f : ldexpf(p, (int)k);     // below 2^-60 the fixed-point weight is 0 anyway
}

__device__ __forceinline__ unsigned long long fixed_weight(float w, float mx) {
    // floor(p * 2^36): the scaling is exact, and so is the split into two 32-bit halves (v < 2^37 carries 24 significant
    // bits: hi = trunc(v 2^-32), v - hi 2^32 is a sub-range of those bits) - two v_cvt_u32_f32 instead of the generic
    // float -> uint64 sequence.  Non-finite weights count 0.
    const float v = isfinite(w) ? exp_spec(w - mx) * 68719476736.0f : 0.f;
    const unsigned hi = (unsigned)(v * 2.3283064365386963e-10f);
    const unsigned lo = (unsigned)(v - (float)hi * 4294967296.0f);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long v, int off) {
    const unsigned lo = __shfl_up((unsigned)v, off), hi = __shfl_up((unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
    const unsigned lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ long shfl_i64(long v, int src) { return (long)shfl_u64((unsigned long long)v, src); }

// stratum map of the systematic resampler (see the fused path in resample_emit.hip and oracle/numerical.py:systematic_strata)
struct Strata {            // t_k = (k * S + U) >> F
    unsigned long long total, S, U;
    int F;
};

__device__ __forceinline__ Strata make_strata(unsigned long long total, double u0, long ns) {
    Strata m;
    m.total = total;
    m.F = total ? __clzll((long long)total) - 2 : 0;           // 62 - bit_length(total)
    m.S = total ? (total << m.F) / (unsigned long long)ns : 0ull;
    unsigned long long U = (unsigned long long)floor(u0 * (double)m.S);
    m.U = (m.S && U > m.S - 1ull) ? m.S - 1ull : U;
    return m;
}
__device__ __forceinline__ Strata load_strata(const unsigned long long* p) {
    Strata m;
    m.total = p[0]; m.S = p[1]; m.U = p[2]; m.F = (int)p[3];
    return m;
}

// the counter hash of the seeded resamplers (splitmix64): spacings, stratum offsets and shuffle keys are pure functions of (seed, i)
constexpr unsigned long long MS_GOLDEN = 0x9E3779B97F4A7C15ull, MS_MIX1 = 0xBF58476D1CE4E5B9ull, MS_MIX2 = 0x94D049BB133111EBull;
__device__ __forceinline__ unsigned long long ms_hash(unsigned long long seed, unsigned long long i) {
    unsigned long long z = seed + (i + 1ull) * MS_GOLDEN;
    z = (z ^ (z >> 30)) * MS_MIX1;
    z = (z ^ (z >> 27)) * MS_MIX2;
    return z ^ (z >> 31);
}

}  // namespace fab
