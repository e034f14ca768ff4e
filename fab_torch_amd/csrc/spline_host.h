// Host-side functions one spline unit calls in another (spline_tile16.hip, spline_stream.hip) and the ONE
// layout of the spline workspace.  Every launcher enqueues on `st` and returns a FABHIP_* code; none allocates or synchronises.
#pragma once
#include "launch.h"
#include "spline_device.h"

namespace fab {

// The workspace of every spline entry point (launch.h: Bump; fabhip_spline_workspace_bytes = carve(nullptr, ..).bytes).
// Without `with_grad` (density alone, sampling) P is one [B][NFP] block and the blocks behind it are absent (null).
struct SplineWs {
    float* Z;                          // [L + 1][B][D] layer input states: Z[l + 1] = input of layer l, Z[0] = base side
    float* P;                          // [with_grad ? L : 1][B][NFP] conditioner outputs (kept per layer for the reverse sweep)
    float* dP;                         // [B][NFP] cotangent of one layer's conditioner output (fabhip_spline_sample_vjp_tape, which
                                       //   keeps its dP on the tapes, holds the [B] log q row sums of its sampler here)
    float *Ga, *Gb;                    // [B][D] cotangents of the state, ping-pong
    unsigned long long* bits;          // ReLU decision words of the 16x16x4 one-launch kernel, per layer and 16-chain tile
    size_t bytes;                      // 0: B < 0
};
static inline SplineWs carve_spline_ws(void* workspace, const SplineDims& f, long B, bool with_grad) {
    SplineWs w{};
    if (B < 0) return w;
    Bump b{(char*)workspace, 256};
    w.Z = b.take<float>((size_t)(f.L + 1) * B * f.D);
    w.P = b.take<float>((size_t)(with_grad ? f.L : 1) * B * f.NFP);
    if (with_grad) {
        w.dP = b.take<float>((size_t)B * f.NFP);
        w.Ga = b.take<float>((size_t)B * f.D);
        w.Gb = b.take<float>((size_t)B * f.D);
        w.bits = b.take<unsigned long long>((size_t)f.L * ceil_div((int)B, ROWS) * (2 * NWAVE * f.NTWM * 4));
    }
    w.bytes = (size_t)(b.p - (char*)workspace) + 256;
    return w;
}

// spline_stream.hip -------------------------------------------------------------------------------------------------------------
// dev-only stage timeline (FABHIP_OPT_TIMELINE): the device buffer of the s_memtime stamps, zeroed on `st`; null when off
long long* sp_timeline(hipStream_t st);
// the density (+ gradient, + tape) call behind fabhip_spline_log_prob and fabhip_spline_log_prob_tape: validation, workspace, then
// one launch (stream or 16x16x4 kernel) or, with a tape or under FABHIP_OPT_SPLINE_STAGED, the staged pass
int spline_log_prob_impl(const fabhip_spline_flow* flow, const float* x, float* log_q, float* grad_x, int64_t B, float* tape,
                         void* workspace, size_t workspace_bytes, hipStream_t st);

// spline_tile16.hip -------------------------------------------------------------------------------------------------------------
// k_spline_logprob / k_spline_logprob_fast: one launch on 16-chain tiles, any hidden width; `fast` only with grad_x
int spline_logprob_t16(const SplineDims& f, const float* packed, const float* x, float* log_q, float* grad_x, long B,
                       const SplineWs& w, int fast, hipStream_t st);
// the density pass of the per-layer kernels (4 L + 2 launches with grad_x); `tape` (nullable): the training tape, needs grad_x
int spline_log_prob_staged(const SplineDims& f, const float* packed, const float* x, float* log_q, float* grad_x, long B,
                           float* tape, const SplineWs& w, hipStream_t st);

}  // namespace fab
