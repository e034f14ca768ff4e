// Circular / linear-tail rational-quadratic spline COUPLING flow (R9s): the flow family the reference builds for
// alanine dipeptide - normflows `CircularCoupledRationalQuadraticSpline` x n_layers (+ PeriodicShift / PeriodicWrap,
// UniformGaussian base), experiments/make_flow/make_aldp_model.py:57-71,121-134,146-167.  Arithmetic restated in
// oracle/spline.py (normflows is absent from the reference tree: parity unpinned, oracle = specification).
//
// Structure (one C-ABI call enqueues all launches of a density / sampling pass, no host synchronisation):
//   k_spline_net_fwd   conditioner of one coupling layer for a 16-chain tile: periodic features of the identity
//                      coordinates -> ResidualNet (Linear, pre-activation residual block, Linear) on the fp32 matrix
//                      cores (flow_device.h ring GEMMs, weights streamed in MFMA B-operand tiles) -> 3K+1 spline
//                      parameters per transformed coordinate, written to HBM
//   k_spline_apply     element-wise: spline evaluation (log_prob direction) or inversion (sampling direction) of the
//                      transformed coordinates with the conditioner's parameters and of the identity coordinates with
//                      the layer's unconditional parameters; log-det row sums; periodic shift / wrap of the next stage
//   k_spline_apply_bwd reverse-mode through the same maps: d log q / d(input) and the cotangents of the 3K+1
//                      conditioner outputs
//   k_spline_net_bwd   recomputes the conditioner's activations for the tile and back-propagates the parameter
//                      cotangents to the identity coordinates (transposed weight tiles on the matrix cores)
//   k_spline_logprob   ONE launch for log q (+ d log q / dx) on the same 16-chain tiles (below); k_spline_logprob_fast: its
//                      fast-mode twin (bf16 conditioner GEMMs)
// One wave handles one chain in the element-wise kernels (lane = coordinate, D <= 64).
//
// This unit: every spline kernel whose conditioner runs on 16-chain tiles and 16x16x4 MFMAs - the per-layer ("staged") kernels
// behind the sampling direction, the training tape, the sampling direction's VJP and the staged density pass
// (FABHIP_OPT_SPLINE_STAGED; every pass with a tape), and the one-launch density kernel for every hidden width.  They share
// sp_net_hidden and stay in one unit: compiled apart, every caller of a unit passes it the same null `bits` (staged kernels) or
// null `act` (one-launch kernel), and k_spline_net_fwd<*> and k_spline_logprob<4, false> come out with other code.  The
// one-launch kernel on 4x4x1 MFMA streams is spline_stream.hip (spline_r8.h), the packed image spline_pack.hip, what the units
// share spline_device.h.
#include "flow_device.h"
#include "target_device.h"
#include "stream_r8.h"
#include "launch.h"
#include <stdlib.h>

#pragma clang fp contract(off)

#include "spline_device.h"
#include "spline_host.h"

namespace fab {

template <int NTWM>
__global__ __launch_bounds__(NTHREADS) void k_spline_net_fwd(SplineDims f, NetLds l, const float* __restrict__ packed,
                                                             int layer, const float* __restrict__ Z,
                                                             float* __restrict__ P, long B, float* __restrict__ act) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Tid t;
    constexpr int DW = depth_w<NTWM>();
    const float* Lp = packed + (size_t)layer * f.layer_stride;
    const long row0 = (long)blockIdx.x * ROWS;
    sp_load_identity(f, Lp, Z, row0, B, lds + l.o_A0, l.AS, t);
    __syncthreads();
    sp_net_hidden<NTWM>(f, l, Lp, lds, t, act, row0, B);
    const float* X1 = lds + l.o_X1;
    const int per = 4 * NTWM * f.KBW * 256;
    for (int c = 0; c < f.NCH; ++c) {
        f32x4 acc[NTWM];
        sp_gemm<NTWM, DW, true>(X1, l.WS, f.KBW, reinterpret_cast<const float4*>(Lp + f.o_Wf + (size_t)c * per),
                                Lp + f.o_bf + c * f.Wp, t, acc);
#pragma unroll
        for (int i = 0; i < NTWM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long g = row0 + 4 * t.q + r;
                if (g < B) P[g * f.NFP + c * f.Wp + 16 * (t.wave + 4 * i) + t.n] = acc[i][r];
            }
    }
}

// backward of the conditioner: dP [B][NFP] -> contribution to d log q / d(identity coordinates), ADDED into G [B][D]
template <int NTWM>
__global__ __launch_bounds__(NTHREADS) void k_spline_net_bwd(SplineDims f, NetLds l, const float* __restrict__ packed,
                                                             int layer, const float* __restrict__ Z,
                                                             const float* __restrict__ dP, float* __restrict__ G, long B,
                                                             SplineTape tp, const float* __restrict__ act) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Tid t;
    constexpr int DW = depth_w<NTWM>();
    const float* Lp = packed + (size_t)layer * f.layer_stride;
    const float* meta = Lp + f.o_meta;
    const long row0 = (long)blockIdx.x * ROWS;
    float* tl = tp.base ? tp.base + (size_t)layer * tp.layer_stride : nullptr;
    float* A0 = lds + l.o_A0; float* H0 = lds + l.o_H0; float* T = lds + l.o_T;
    float* X1 = lds + l.o_X1; float* X2 = lds + l.o_X2; float* DP = lds + l.o_DP; float* PART = lds + l.o_PART;
    if (!act) sp_load_identity(f, Lp, Z, row0, B, A0, l.AS, t);
    sp_tile_load4(DP, l.PS, dP, f.NFP, f.NFP, row0, B, t);
    if (act) {                                          // the forward kept relu(h0) | relu(t): only their signs matter here
        sp_tile_load4(H0, l.WS, act, 2 * f.Wp, f.Wp, row0, B, t);
        sp_tile_load4(T, l.WS, act + f.Wp, 2 * f.Wp, f.Wp, row0, B, t);
    }
    __syncthreads();
    if (!act) sp_net_hidden<NTWM>(f, l, Lp, lds, t);    // recompute h0 (H0) and t (T): the ReLU decisions
    if (tl) {
        sp_tape_rows(tl + tp.o_A0, 64, A0, l.AS, row0, B, t);
        sp_tape_rows(tl + tp.o_R0, f.Wp, X2, l.WS, row0, B, t);
        sp_tape_rows(tl + tp.o_H1, f.Wp, X1, l.WS, row0, B, t);
        for (int e = t.tid; e < ROWS * f.Wp; e += NTHREADS) {
            const int r = e / f.Wp, c = e % f.Wp;
            if (row0 + r < B) { const float v = T[r * l.WS + c]; tl[tp.o_R1 + (row0 + r) * f.Wp + c] = v > 0.f ? v : 0.f; }
        }
        __syncthreads();
    }
    f32x4 acc[NTWM];
    // dh1 = dP WfT  -> X1
    sp_gemm<NTWM, DW, false>(DP, l.PS, f.NFP / 16, reinterpret_cast<const float4*>(Lp + f.o_WfT), nullptr, t, acc);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NTWM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) X1[(4 * t.q + r) * l.WS + 16 * (t.wave + 4 * i) + t.n] = acc[i][r];
    __syncthreads();
    if (tl) sp_tape_rows(tl + tp.o_dH1, f.Wp, X1, l.WS, row0, B, t);
    // d relu(t) = dh1 WbT, masked by t > 0 -> X2
    sp_gemm<NTWM, DW, false>(X1, l.WS, f.KBW, reinterpret_cast<const float4*>(Lp + f.o_WbT), nullptr, t, acc);
#pragma unroll
    for (int i = 0; i < NTWM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (4 * t.q + r) * l.WS + 16 * (t.wave + 4 * i) + t.n;
            X2[o] = T[o] > 0.f ? acc[i][r] : 0.f;
        }
    __syncthreads();
    if (tl) sp_tape_rows(tl + tp.o_dT, f.Wp, X2, l.WS, row0, B, t);
    // dh0 = dh1 + (dt WaT) masked by h0 > 0 -> T
    sp_gemm<NTWM, DW, false>(X2, l.WS, f.KBW, reinterpret_cast<const float4*>(Lp + f.o_WaT), nullptr, t, acc);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NTWM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (4 * t.q + r) * l.WS + 16 * (t.wave + 4 * i) + t.n;
            T[o] = X1[o] + (H0[o] > 0.f ? acc[i][r] : 0.f);
        }
    __syncthreads();
    if (tl) sp_tape_rows(tl + tp.o_dH0, f.Wp, T, l.WS, row0, B, t);
    // dA0 = dh0 W0T (N = 64: K-split over the waves)
    gemm_ksplit<NTWM>(T, l.WS, reinterpret_cast<const float4*>(Lp + f.o_W0T), 4, PART, l.AS, t);
    __syncthreads();
    const int n_id = (int)meta[M_CNT * 64];
    for (int e = t.tid; e < ROWS * 64; e += NTHREADS) {
        const int r = e >> 6, i = e & 63;
        const long g = row0 + r;
        if (tl && g < B && i >= n_id) { tl[tp.o_XI + g * 64 + i] = 0.f; tl[tp.o_dA0 + g * 64 + i] = 0.f; }
        if (i < n_id && g < B) {
            float d = part_sum(PART, l.AS, r, i);
            const int feat = (int)meta[M_IDF * 64 + i];
            if (tl) { tl[tp.o_XI + g * 64 + i] = Z[g * f.D + feat]; tl[tp.o_dA0 + g * 64 + i] = d; }
            if (meta[M_PFON * 64 + i] != 0.f) {
                const int k = (int)meta[M_PFK * 64 + i];
                const float s = meta[M_PFS * 64 + i], x = Z[g * f.D + feat];
                d = d * (s * (Lp[f.o_pfw + 2 * k] * cosf(s * x) - Lp[f.o_pfw + 2 * k + 1] * sinf(s * x)));
            }
            G[g * f.D + feat] += d;
        }
    }
}

// One wave per chain, lane = coordinate.  MODE 0: log_prob direction (evaluate), 1: sampling direction, identity
// coordinates only (unconditional inverse, before the conditioner runs), 2: sampling direction, transformed
// coordinates (needs P) + post shift (Ypre, nullable: the state before that shift, kept for fabhip_spline_sample_vjp_tape).
template <int MODE>
__global__ __launch_bounds__(256) void k_spline_apply(SplineDims f, const float* __restrict__ packed, int layer,
                                                      const float* __restrict__ Zin, const float* __restrict__ P,
                                                      float* __restrict__ Zout, float* __restrict__ log_q, float ld_sign,
                                                      long B, float* __restrict__ Ypre) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= B) return;
    const float* Lp = packed + (size_t)layer * f.layer_stride;
    const float* meta = Lp + f.o_meta;
    const int n_id = (int)meta[M_CNT * 64], n_tr = (int)meta[M_CNT * 64 + 1];
    const float isq = 1.f / sqrtf((float)f.W);
    float ld = 0.f;
    if (lane < f.D) {
        // role of this coordinate
        const int pos_id = (int)meta[M_POSID * 64 + lane], pos_tr = (int)meta[M_POSTR * 64 + lane];
        const bool circ = meta[M_CIRC * 64 + lane] != 0.f;
        const float tb = meta[M_TB * 64 + lane];
        float z = Zin[g * f.D + lane], out = z;
        float p[SP_NP];
        Rqs s;
        if (pos_id >= 0 && MODE != 2) {
#pragma unroll
            for (int j = 0; j < SP_NP; ++j) p[j] = Lp[f.o_unc + pos_id * SP_NP + j];
            rqs_setup(p, circ, tb, s);
            float l1;
            if (MODE == 0) rqs_forward(s, z, tb, out, l1); else rqs_inverse(s, z, tb, out, l1);
            ld = l1;
        } else if (pos_tr >= 0 && MODE != 1) {
#pragma unroll
            for (int j = 0; j < SP_NP; ++j) {
                const float v = P[g * f.NFP + pos_tr * SP_NP + j];
                p[j] = j < 2 * SP_K ? v * isq : v;
            }
            rqs_setup(p, circ, tb, s);
            float l1;
            if (MODE == 0) rqs_forward(s, z, tb, out, l1); else rqs_inverse(s, z, tb, out, l1);
            ld = l1;
        }
        // stage boundary: MODE 0 -> the NEXT (lower) layer's pre-shift; MODE 2 -> this layer's post-shift
        if (MODE == 0 && layer > 0) {
            const float* mn = packed + (size_t)(layer - 1) * f.layer_stride + f.o_meta;
            if (mn[M_PREON * 64 + lane] != 0.f) out = sp_wrap(out - mn[M_PRESH * 64 + lane], tb);
        }
        if (MODE == 2 && Ypre) Ypre[g * f.D + lane] = out;         // the layer's output before the shift = the log_prob direction's input
        if (MODE == 2 && meta[M_POSTON * 64 + lane] != 0.f) out = sp_wrap(out + meta[M_POSTSH * 64 + lane], tb);
        Zout[g * f.D + lane] = out;
    }
    ld = wave_sum64(ld);
    if (lane == 0) log_q[g] += ld_sign * ld;
}

// x <- wrap(x - pre_shift of the top layer) : the first stage of the log_prob direction (PeriodicWrap.inverse)
__global__ void k_spline_first_stage(SplineDims f, const float* __restrict__ packed, const float* __restrict__ x,
                                     float* __restrict__ Z, float* __restrict__ log_q, long B) {
    const float* meta = packed + (size_t)(f.L - 1) * f.layer_stride + f.o_meta;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < B * f.D; e += (long)gridDim.x * blockDim.x) {
        const int j = (int)(e % f.D);
        float v = x[e];
        if (meta[M_PREON * 64 + j] != 0.f) v = sp_wrap(v - meta[M_PRESH * 64 + j], meta[M_TB * 64 + j]);
        Z[e] = v;
        if (j == 0) log_q[e / f.D] = 0.f;
    }
}

// base UniformGaussian: log_q += log p0(z); G = d log p0 / dz (if G)
__global__ __launch_bounds__(256) void k_spline_base(SplineDims f, const float* __restrict__ packed,
                                                     const float* __restrict__ Z, float* __restrict__ log_q,
                                                     float* __restrict__ G, long B) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= B) return;
    float lp = 0.f;
    if (lane < f.D) {
        const float sc = packed[f.o_base + lane];
        const bool circ = packed[f.o_base + 64 + lane] != 0.f;
        const float z = Z[g * f.D + lane];
        if (circ) { lp = -logf(sc); if (G) G[g * f.D + lane] = 0.f; }
        else {
            lp = -0.5f * 1.8378770664093453f - logf(sc) - 0.5f * ((z / sc) * (z / sc));
            if (G) G[g * f.D + lane] = -(z / sc) / sc;
        }
    }
    lp = wave_sum64(lp);
    if (lane == 0) log_q[g] += lp;
}

// sampling: z0 = base sample from (u, eps), log_q = log p0(z0)
__global__ __launch_bounds__(256) void k_spline_base_sample(SplineDims f, const float* __restrict__ packed,
                                                            const float* __restrict__ u, const float* __restrict__ eps,
                                                            float* __restrict__ Z, float* __restrict__ log_q, long B) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= B) return;
    float lp = 0.f;
    if (lane < f.D) {
        const float sc = packed[f.o_base + lane];
        const bool circ = packed[f.o_base + 64 + lane] != 0.f;
        const float z = (circ ? u[g * f.D + lane] - 0.5f : eps[g * f.D + lane]) * sc;
        Z[g * f.D + lane] = z;
        lp = circ ? -logf(sc) : -0.5f * 1.8378770664093453f - logf(sc) - 0.5f * ((z / sc) * (z / sc));
    }
    lp = wave_sum64(lp);
    if (lane == 0) log_q[g] = lp;
}

// reverse mode through k_spline_apply<0> of one layer: Gout (cotangent of the layer's output state, BEFORE the stage
// boundary shift, which has unit derivative) -> Gin (w.r.t. the layer's input state, conditioner path excluded) and dP
__global__ __launch_bounds__(256) void k_spline_apply_bwd(SplineDims f, const float* __restrict__ packed, int layer,
                                                          const float* __restrict__ Zin, const float* __restrict__ P,
                                                          const float* __restrict__ Gout, float* __restrict__ Gin,
                                                          float* __restrict__ dP, long B, float* __restrict__ dU) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= B) return;
    const float* Lp = packed + (size_t)layer * f.layer_stride;
    const float* meta = Lp + f.o_meta;
    const int n_id = (int)meta[M_CNT * 64], n_tr = (int)meta[M_CNT * 64 + 1];
    const float isq = 1.f / sqrtf((float)f.W);
    // zero the padding columns of this chain's dP row (the conditioner backward reads all NFP of them)
    for (int j = n_tr * SP_NP + lane; j < f.NFP; j += 64) dP[g * f.NFP + j] = 0.f;
    if (lane >= f.D) return;
    const int pos_id = (int)meta[M_POSID * 64 + lane], pos_tr = (int)meta[M_POSTR * 64 + lane];
    const bool circ = meta[M_CIRC * 64 + lane] != 0.f;
    const float tb = meta[M_TB * 64 + lane];
    const float z = Zin[g * f.D + lane], gy = Gout[g * f.D + lane];
    float p[SP_NP];
    Rqs s;
    float gx = gy;
    if (pos_id >= 0) {
#pragma unroll
        for (int j = 0; j < SP_NP; ++j) p[j] = Lp[f.o_unc + pos_id * SP_NP + j];
        rqs_setup(p, circ, tb, s);
        if (dU) {
            float dp[SP_NP];
            gx = rqs_backward(s, p, circ, z, tb, gy, 1.f, dp);
#pragma unroll
            for (int j = 0; j < SP_NP; ++j) dU[g * (SP_MD * SP_NP) + pos_id * SP_NP + j] = dp[j];
        } else {
            gx = rqs_backward(s, p, circ, z, tb, gy, 1.f, nullptr);
        }
    } else if (pos_tr >= 0) {
#pragma unroll
        for (int j = 0; j < SP_NP; ++j) {
            const float v = P[g * f.NFP + pos_tr * SP_NP + j];
            p[j] = j < 2 * SP_K ? v * isq : v;
        }
        rqs_setup(p, circ, tb, s);
        float dp[SP_NP];
        gx = rqs_backward(s, p, circ, z, tb, gy, isq, dp);
#pragma unroll
        for (int j = 0; j < SP_NP; ++j) dP[g * f.NFP + pos_tr * SP_NP + j] = dp[j];
    }
    Gin[g * f.D + lane] = gx;
}

// Sampling-direction gradients (x = S^-1(z0; theta) with the noise z0 fixed, S = the log_prob direction): for a cotangent gx of
// x and gl of log q(x), d/d theta = gl d log q / d theta |_x  -  v^T dS / d theta with v = (dS / dx)^-T (gx + gl d log q / dx)
// (implicit function theorem).  The first term is the density tape's; this kernel carries v through ONE coupling layer
// y -> z = (g_u(y_id), g(y_tr; c(y_id))) from the x side to the base side and leaves  -v_z dz / d(parameters)  where the
// density tape keeps its parameter cotangents, so the SAME conditioner backward and the SAME tape GEMMs finish the job:
//   PART 0 (before the conditioner backward): transformed coordinates  v_z = v_y / g'(y),  dP = -v_z dg / dP;  identity
//          coordinates copied (the conditioner backward then ADDS  -A^T v_z,tr  to them, A = dg / dy_id through the net)
//   PART 1 (after it): identity coordinates  v_z = (v_y - A^T v_z,tr) / g_u'(y),  dU = -v_z dg_u / dU
// v = gx + gl * (d log q / dx), in place in v (gx / gl nullable: a cotangent that is not there)
__global__ void k_spline_vjp_seed(float* __restrict__ v, const float* __restrict__ gx, const float* __restrict__ gl, long B, int D) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < B * D; e += (long)gridDim.x * blockDim.x)
        v[e] = (gx ? gx[e] : 0.f) + (gl ? gl[e / D] * v[e] : 0.f);
}

template <int PART>
__global__ __launch_bounds__(256) void k_spline_vsweep(SplineDims f, const float* __restrict__ packed, int layer,
                                                       const float* __restrict__ Zin, const float* __restrict__ P,
                                                       const float* __restrict__ Vin, float* __restrict__ Vout,
                                                       float* __restrict__ dP, long B, float* __restrict__ dU) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= B) return;
    const float* Lp = packed + (size_t)layer * f.layer_stride;
    const float* meta = Lp + f.o_meta;
    const int n_tr = (int)meta[M_CNT * 64 + 1];
    const float isq = 1.f / sqrtf((float)f.W);
    if (PART == 0)
        for (int j = n_tr * SP_NP + lane; j < f.NFP; j += 64) dP[g * f.NFP + j] = 0.f;
    if (lane >= f.D) return;
    const int pos_id = (int)meta[M_POSID * 64 + lane], pos_tr = (int)meta[M_POSTR * 64 + lane];
    const bool circ = meta[M_CIRC * 64 + lane] != 0.f;
    const float tb = meta[M_TB * 64 + lane];
    const float y = Zin[g * f.D + lane];
    float p[SP_NP], dp[SP_NP];
    Rqs s;
    if (PART == 0) {
        float v = Vin[g * f.D + lane];
        if (pos_tr >= 0) {
#pragma unroll
            for (int j = 0; j < SP_NP; ++j) {
                const float c = P[g * f.NFP + pos_tr * SP_NP + j];
                p[j] = j < 2 * SP_K ? c * isq : c;
            }
            rqs_setup(p, circ, tb, s);
            v = v / rqs_backward<false>(s, p, circ, y, tb, 1.f, isq, nullptr);
            rqs_backward<false>(s, p, circ, y, tb, -v, isq, dp);
#pragma unroll
            for (int j = 0; j < SP_NP; ++j) dP[g * f.NFP + pos_tr * SP_NP + j] = dp[j];
        }
        Vout[g * f.D + lane] = v;
    } else if (pos_id >= 0) {
#pragma unroll
        for (int j = 0; j < SP_NP; ++j) p[j] = Lp[f.o_unc + pos_id * SP_NP + j];
        rqs_setup(p, circ, tb, s);
        const float v = Vout[g * f.D + lane] / rqs_backward<false>(s, p, circ, y, tb, 1.f, 1.f, nullptr);
        rqs_backward<false>(s, p, circ, y, tb, -v, 1.f, dp);
#pragma unroll
        for (int j = 0; j < SP_NP; ++j) dU[g * (SP_MD * SP_NP) + pos_id * SP_NP + j] = dp[j];
        Vout[g * f.D + lane] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// ONE launch for log q (+ d log q / dx): a workgroup carries its 16 chains through all layers - conditioner on the
// matrix cores, its 3K+1 parameters per coordinate kept in LDS, the splines evaluated by the same workgroup (thread =
// (chain, coordinate mod 16)), the state tile never leaving LDS - then, with GRAD, back again (layer inputs, conditioner
// outputs and ReLU decisions of the forward sweep are parked in the workspace, per tile: L2-resident).  Replaces 4 L + 2
// launches of the per-stage kernels above (kept for the training tape and the sampling direction).
// ------------------------------------------------------------------------------------------------
template <int NTWM, bool GRAD, bool FAST>
__device__ __forceinline__ void spline_logprob_body(const SplineDims& f, const NetLds& l, const float* __restrict__ packed,
                                                    const float* __restrict__ x, float* __restrict__ log_q,
                                                    float* __restrict__ grad_x, long B, float* __restrict__ Zsave,
                                                    float* __restrict__ Psave, unsigned long long* __restrict__ bitsave, float* lds,
                                                    long long* tlp = nullptr) {
    Tid t;
#define SP_TL(idx) do { if (tlp && blockIdx.x == 0 && threadIdx.x == 0) tlp[idx] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
    constexpr int DW = depth_w<NTWM>();
    const long row0 = (long)blockIdx.x * ROWS;
    float* A0 = lds + l.o_A0; float* H0 = lds + l.o_H0; float* T = lds + l.o_T;
    float* X1 = lds + l.o_X1; float* X2 = lds + l.o_X2; float* PT = lds + l.o_DP; float* PART = lds + l.o_PART;
    float* ZT = lds + l.o_ZT; float* GT = lds + l.o_GT;
    const float isq = 1.f / sqrtf((float)f.W);
    const int per = 4 * NTWM * f.KBW * 256;
    const size_t zs = (size_t)B * f.D, ps = (size_t)B * f.NFP;
    // x <- wrap(x - pre-shift of the top layer)   (PeriodicWrap.inverse / the last PeriodicShift.inverse)
    {
        const float* mt = packed + (size_t)(f.L - 1) * f.layer_stride + f.o_meta;
        for (int e = t.tid; e < ROWS * 64; e += NTHREADS) {
            const int r = e >> 6, j = e & 63;
            const long g = row0 + r;
            float v = 0.f;
            if (j < f.D && g < B) {
                v = x[g * f.D + j];
                if (mt[M_PREON * 64 + j] != 0.f) v = sp_wrap(v - mt[M_PRESH * 64 + j], mt[M_TB * 64 + j]);
            }
            ZT[e] = v;
        }
    }
    __syncthreads();
    float ld_acc = 0.f;
    for (int layer = f.L - 1; layer >= 0; --layer) {
        const float* Lp = packed + (size_t)layer * f.layer_stride;
        const float* meta = Lp + f.o_meta;
        const bool tl = layer == 1;
        if (tl) SP_TL(0);
        if (GRAD) {                                        // this layer's input state, for the reverse sweep
            for (int e = t.tid; e < ROWS * f.D; e += NTHREADS) {
                const int r = e / f.D, j = e % f.D;
                if (row0 + r < B) Zsave[(size_t)layer * zs + (row0 + r) * f.D + j] = ZT[r * 64 + j];
            }
        }
        sp_identity_from_tile(f, Lp, ZT, A0, l.AS, t);
        __syncthreads();
        if (tl) SP_TL(1);
        sp_net_hidden<NTWM, FAST>(f, l, Lp, lds, t, nullptr, row0, B,
                                  GRAD ? bitsave + ((size_t)layer * gridDim.x + blockIdx.x) * (2 * NWAVE * NTWM * 4) : nullptr);
        if (tl) SP_TL(2);
        for (int c = 0; c < f.NCH; ++c) {
            f32x4 acc[NTWM];
            if constexpr (FAST) sp_gemm_bf16<NTWM, true>(f, X1, l.WS, Lp, 2 + c, Lp + f.o_bf + c * f.Wp, t, acc);
            else sp_gemm<NTWM, DW, true>(X1, l.WS, f.KBW, reinterpret_cast<const float4*>(Lp + f.o_Wf + (size_t)c * per),
                                         Lp + f.o_bf + c * f.Wp, t, acc);
#pragma unroll
            for (int i = 0; i < NTWM; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = c * f.Wp + 16 * (t.wave + 4 * i) + t.n;
                    PT[(4 * t.q + r) * l.PS + col] = acc[i][r];
                }
        }
        __syncthreads();
        if (GRAD) sp_tile_store4(Psave + (size_t)layer * ps, f.NFP, PT, l.PS, f.NFP, row0, B, t);   // for the reverse sweep
        if (tl) SP_TL(3);
        const float* mn = layer > 0 ? packed + (size_t)(layer - 1) * f.layer_stride + f.o_meta : nullptr;
        for (int j = t.c; j < f.D; j += 16) {
            float p[SP_NP];
            int pos;
            const int kind = sp_coord_params(f, Lp, meta, PT, l.PS, t.row, j, isq, p, pos);
            const float tb = meta[M_TB * 64 + j];
            float out = ZT[t.row * 64 + j];
            if (kind) {
                Rqs sp;
                rqs_setup(p, meta[M_CIRC * 64 + j] != 0.f, tb, sp);
                float l1;
                rqs_forward(sp, out, tb, out, l1);
                ld_acc += l1;
            }
            if (mn && mn[M_PREON * 64 + j] != 0.f) out = sp_wrap(out - mn[M_PRESH * 64 + j], tb);   // next stage's shift
            ZT[t.row * 64 + j] = out;
        }
        __syncthreads();
        if (tl) SP_TL(4);
    }
    // base UniformGaussian
    for (int j = t.c; j < f.D; j += 16) {
        const float sc = packed[f.o_base + j];
        const float z = ZT[t.row * 64 + j];
        if (packed[f.o_base + 64 + j] != 0.f) { ld_acc += -logf(sc); if (GRAD) GT[t.row * 64 + j] = 0.f; }
        else {
            ld_acc += -0.5f * 1.8378770664093453f - logf(sc) - 0.5f * ((z / sc) * (z / sc));
            if (GRAD) GT[t.row * 64 + j] = -(z / sc) / sc;
        }
    }
    const float lq = row16_sum(ld_acc);
    if (t.c == 0 && row0 + t.row < B) log_q[row0 + t.row] = lq;
    if (!GRAD) return;
    __syncthreads();
    // ---- reverse sweep: GT = d log q / d(state), layers 0 .. L-1 ---------------------------------------------------
    for (int layer = 0; layer < f.L; ++layer) {
        const float* Lp = packed + (size_t)layer * f.layer_stride;
        const float* meta = Lp + f.o_meta;
        const int n_id = (int)meta[M_CNT * 64], n_tr = (int)meta[M_CNT * 64 + 1];
        const bool tl = layer == 1;
        if (tl) SP_TL(8);
        for (int e = t.tid; e < ROWS * 64; e += NTHREADS) {           // layer input state
            const int r = e >> 6, j = e & 63;
            ZT[e] = (j < f.D && row0 + r < B) ? Zsave[(size_t)layer * zs + (row0 + r) * f.D + j] : 0.f;
        }
        // conditioner output (-> dP in place below) and the ReLU decisions of the forward sweep
        sp_tile_load4(PT, l.PS, Psave + (size_t)layer * ps, f.NFP, f.NFP, row0, B, t);
        unsigned long long m0[NTWM][4], m1[NTWM][4];                       // this thread's ReLU decisions (wave-uniform words)
        {
            const unsigned long long* bw = bitsave + ((size_t)layer * gridDim.x + blockIdx.x) * (2 * NWAVE * NTWM * 4);
#pragma unroll
            for (int i = 0; i < NTWM; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    m0[i][r] = bw[((0 * NWAVE + t.wave) * NTWM + i) * 4 + r];
                    m1[i][r] = bw[((1 * NWAVE + t.wave) * NTWM + i) * 4 + r];
                }
        }
        __syncthreads();
        if (tl) SP_TL(9);
        for (int j = t.c; j < f.D; j += 16) {
            float p[SP_NP];
            int pos;
            const int kind = sp_coord_params(f, Lp, meta, PT, l.PS, t.row, j, isq, p, pos);
            if (kind) {
                const float tb = meta[M_TB * 64 + j];
                const bool circ = meta[M_CIRC * 64 + j] != 0.f;
                Rqs sp;
                rqs_setup(p, circ, tb, sp);
                const float z = ZT[t.row * 64 + j], gy = GT[t.row * 64 + j];
                if (kind == 2) {
                    float dp[SP_NP];
                    GT[t.row * 64 + j] = rqs_backward(sp, p, circ, z, tb, gy, isq, dp);
#pragma unroll
                    for (int k = 0; k < SP_NP; ++k) PT[t.row * l.PS + pos * SP_NP + k] = dp[k];
                } else {
                    GT[t.row * 64 + j] = rqs_backward(sp, p, circ, z, tb, gy, 1.f, nullptr);
                }
            }
        }
        for (int c = n_tr * SP_NP + t.c; c < l.PS; c += 16) PT[t.row * l.PS + c] = 0.f;    // padding columns of dP
        __syncthreads();
        if (tl) SP_TL(10);
        f32x4 acc[NTWM];
        if constexpr (FAST) {                              // K = NFP: NCH slices of K = Wp of the WfT image
#pragma unroll
            for (int i = 0; i < NTWM; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const uint4* Bh = reinterpret_cast<const uint4*>(Lp + f.o_h + (size_t)(2 + f.NCH) * (f.Wp * f.Wp / 2));
            for (int c = 0; c < f.NCH; ++c) gemm_bf16_slice<NTWM>(PT, l.PS, Bh, f.NFP / 32, c * (f.Wp / 32), t, acc);
        } else {
            sp_gemm<NTWM, DW, false>(PT, l.PS, f.NFP / 16, reinterpret_cast<const float4*>(Lp + f.o_WfT), nullptr, t, acc);
        }
#pragma unroll
        for (int i = 0; i < NTWM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) X1[(4 * t.q + r) * l.WS + 16 * (t.wave + 4 * i) + t.n] = acc[i][r];
        __syncthreads();
        if (tl) SP_TL(11);
        if constexpr (FAST) sp_gemm_bf16<NTWM, false>(f, X1, l.WS, Lp, 2 + 2 * f.NCH, nullptr, t, acc);
        else sp_gemm<NTWM, DW, false>(X1, l.WS, f.KBW, reinterpret_cast<const float4*>(Lp + f.o_WbT), nullptr, t, acc);
#pragma unroll
        for (int i = 0; i < NTWM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = (4 * t.q + r) * l.WS + 16 * (t.wave + 4 * i) + t.n;
                X2[o] = ((m1[i][r] >> t.lane) & 1ull) ? acc[i][r] : 0.f;
            }
        __syncthreads();
        if constexpr (FAST) sp_gemm_bf16<NTWM, false>(f, X2, l.WS, Lp, 3 + 2 * f.NCH, nullptr, t, acc);
        else sp_gemm<NTWM, DW, false>(X2, l.WS, f.KBW, reinterpret_cast<const float4*>(Lp + f.o_WaT), nullptr, t, acc);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NTWM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = (4 * t.q + r) * l.WS + 16 * (t.wave + 4 * i) + t.n;
                T[o] = X1[o] + (((m0[i][r] >> t.lane) & 1ull) ? acc[i][r] : 0.f);
            }
        __syncthreads();
        if (tl) SP_TL(12);
        gemm_ksplit<NTWM>(T, l.WS, reinterpret_cast<const float4*>(Lp + f.o_W0T), 4, PART, l.AS, t);
        __syncthreads();
        if (tl) SP_TL(13);
        for (int e = t.tid; e < ROWS * 64; e += NTHREADS) {
            const int r = e >> 6, i = e & 63;
            if (i < n_id) {
                float d = part_sum(PART, l.AS, r, i);
                const int feat = (int)meta[M_IDF * 64 + i];
                if (meta[M_PFON * 64 + i] != 0.f) {
                    const int k = (int)meta[M_PFK * 64 + i];
                    const float sc = meta[M_PFS * 64 + i], zz = ZT[r * 64 + feat];
                    d = d * (sc * (Lp[f.o_pfw + 2 * k] * cosf(sc * zz) - Lp[f.o_pfw + 2 * k + 1] * sinf(sc * zz)));
                }
                GT[r * 64 + feat] += d;
            }
        }
        __syncthreads();
        if (tl) SP_TL(14);
    }
    for (int e = t.tid; e < ROWS * f.D; e += NTHREADS) {
        const int r = e / f.D, j = e % f.D;
        if (row0 + r < B) grad_x[(row0 + r) * f.D + j] = GT[r * 64 + j];
    }
#undef SP_TL
}

template <int NTWM, bool GRAD>
__global__ __launch_bounds__(NTHREADS) void k_spline_logprob(SplineDims f, NetLds l, const float* __restrict__ packed,
                                                             const float* __restrict__ x, float* __restrict__ log_q,
                                                             float* __restrict__ grad_x, long B,
                                                             float* __restrict__ Zsave, float* __restrict__ Psave,
                                                             unsigned long long* __restrict__ bitsave, long long* tlp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    spline_logprob_body<NTWM, GRAD, false>(f, l, packed, x, log_q, grad_x, B, Zsave, Psave, bitsave, lds, tlp);
}
// fast mode (fabhip_set_fast_mode): the conditioner's Wp x Wp GEMMs on the bf16 matrix cores; gradient evaluations only
template <int NTWM>
__global__ __launch_bounds__(NTHREADS) void k_spline_logprob_fast(SplineDims f, NetLds l, const float* __restrict__ packed,
                                                                  const float* __restrict__ x, float* __restrict__ log_q,
                                                                  float* __restrict__ grad_x, long B,
                                                                  float* __restrict__ Zsave, float* __restrict__ Psave,
                                                                  unsigned long long* __restrict__ bitsave, long long* tlp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    spline_logprob_body<NTWM, true, true>(f, l, packed, x, log_q, grad_x, B, Zsave, Psave, bitsave, lds, tlp);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// the one-launch kernel: density alone, with its gradient, or with its gradient in fast mode
template <int NTWM>
static int launch_logprob(const SplineDims& f, const float* packed, const float* x, float* log_q, float* grad_x, long B,
                          const SplineWs& w, int fast, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div((int)B, ROWS)), block(NTHREADS);
    const NetLds l = make_net_lds(f, grad_x != nullptr, true);
    const size_t bytes = (size_t)l.total * 4;
    long long* tl = sp_timeline(st);                       // (enqueues its memset: in front of the kernel)
    if (grad_x && fast)
        return launch_lds(k_spline_logprob_fast<NTWM>, grid, block, bytes, st, f, l, packed, x, log_q, grad_x, B, w.Z, w.P, w.bits, tl);
    if (grad_x)
        return launch_lds(k_spline_logprob<NTWM, true>, grid, block, bytes, st, f, l, packed, x, log_q, grad_x, B, w.Z, w.P, w.bits, tl);
    return launch_lds(k_spline_logprob<NTWM, false>, grid, block, bytes, st, f, l, packed, x, log_q, grad_x, B, w.Z, w.P, w.bits, tl);
}

int spline_logprob_t16(const SplineDims& f, const float* packed, const float* x, float* log_q, float* grad_x, long B,
                       const SplineWs& w, int fast, hipStream_t st) {
    if (f.NTWM == 1) return launch_logprob<1>(f, packed, x, log_q, grad_x, B, w, fast, st);
    if (f.NTWM == 2) return launch_logprob<2>(f, packed, x, log_q, grad_x, B, w, fast, st);
    if (f.NTWM == 4) return launch_logprob<4>(f, packed, x, log_q, grad_x, B, w, fast, st);
    return FABHIP_ENOTSUP;
}

template <int NTWM>
static int launch_net(const SplineDims& f, const float* packed, int layer, const float* Z, float* P, const float* dP,
                      float* G, long B, hipStream_t st, const SplineTape& tp, float* act) {
    const dim3 grid((unsigned)ceil_div((int)B, ROWS)), block(NTHREADS);
    const bool bwd = dP != nullptr;
    const NetLds l = make_net_lds(f, bwd);
    const size_t bytes = (size_t)l.total * 4;
    if (bwd)
        return launch_lds(k_spline_net_bwd<NTWM>, grid, block, bytes, st, f, l, packed, layer, Z, dP, G, B, tp,
                          tp.base ? nullptr : act);
    return launch_lds(k_spline_net_fwd<NTWM>, grid, block, bytes, st, f, l, packed, layer, Z, P, B, act);
}

// the conditioner of one layer: forward (P) or, with dP, backward (ADDED into G; `tp.base`: + the layer's tape rows)
static int net(const SplineDims& f, const float* packed, int layer, const float* Z, float* P, const float* dP, float* G,
               long B, hipStream_t st, const SplineTape& tp = SplineTape{}, float* act = nullptr) {
    if (f.NTWM == 1) return launch_net<1>(f, packed, layer, Z, P, dP, G, B, st, tp, act);
    if (f.NTWM == 2) return launch_net<2>(f, packed, layer, Z, P, dP, G, B, st, tp, act);
    if (f.NTWM == 4) return launch_net<4>(f, packed, layer, Z, P, dP, G, B, st, tp, act);
    return FABHIP_ENOTSUP;
}

// grid of the grid-stride element-wise kernels over n elements: 256 threads each, at most 4096 workgroups
static inline dim3 elementwise_grid(long n) {
    const long g = (n + 255) / 256;
    return dim3((unsigned)(g > 4096 ? 4096 : g));
}

int spline_log_prob_staged(const SplineDims& f, const float* pk, const float* x, float* log_q, float* grad_x, long B,
                           float* tape, const SplineWs& w, hipStream_t st) {
    float* Z = w.Z; float* P = w.P;
    const size_t zs = (size_t)B * f.D, ps = (size_t)B * f.NFP;
    const SplineTape tp = make_spline_tape(f, B, tape);
    const dim3 wgrid((unsigned)((B + 3) / 4)), wblock(256);
    hipLaunchKernelGGL(k_spline_first_stage, elementwise_grid(B * f.D), dim3(256), 0, st, f, pk, x, Z + (size_t)f.L * zs, log_q, B);
    for (int l = f.L - 1; l >= 0; --l) {
        float* Pl = P + (grad_x ? (size_t)l * ps : 0);
        FAB_TRY(net(f, pk, l, Z + (size_t)(l + 1) * zs, Pl, nullptr, nullptr, B, st));
        hipLaunchKernelGGL(k_spline_apply<0>, wgrid, wblock, 0, st, f, pk, l, Z + (size_t)(l + 1) * zs, Pl, Z + (size_t)l * zs,
                           log_q, 1.f, B, (float*)nullptr);
    }
    hipLaunchKernelGGL(k_spline_base, wgrid, wblock, 0, st, f, pk, Z, log_q, w.Ga, B);
    if (grad_x) {
        float* gin = w.Ga;                               // cotangent of Z[0] (the base side): d log p0 / dz
        for (int l = 0; l < f.L; ++l) {
            float* out = (l == f.L - 1) ? grad_x : (gin == w.Ga ? w.Gb : w.Ga);
            float* dPl = tape ? tape + (size_t)l * tp.layer_stride + tp.o_dP : w.dP;    // kept per layer on the tape
            float* dUl = tape ? tape + (size_t)l * tp.layer_stride + tp.o_dU : nullptr;
            hipLaunchKernelGGL(k_spline_apply_bwd, wgrid, wblock, 0, st, f, pk, l, Z + (size_t)(l + 1) * zs,
                               P + (size_t)l * ps, gin, out, dPl, B, dUl);
            FAB_TRY(net(f, pk, l, Z + (size_t)(l + 1) * zs, nullptr, dPl, out, B, st, tp));
            gin = out;
        }
    }
    return check_launch();
}

}  // namespace fab

using namespace fab;

extern "C" {

int fabhip_spline_tape_layout(int32_t dim, int32_t n_layers, int32_t hidden, int64_t B, int64_t out16[16]) {
    if (!out16 || B < 0) return FABHIP_EINVAL;
    FAB_TRY(check_spline_shape(dim, n_layers, hidden));
    const SplineDims f = make_spline_dims(dim, n_layers, hidden);
    const SplineTape t = make_spline_tape(f, (long)B, nullptr);
    const int64_t v[16] = {(int64_t)t.layer_stride * n_layers, t.layer_stride, t.o_XI, t.o_A0, t.o_dA0, t.o_R0, t.o_R1, t.o_H1,
                           t.o_dH1, t.o_dT, t.o_dH0, t.o_dP, t.o_dU, f.Wp, f.NFP, SP_MD * SP_NP};
    for (int i = 0; i < 16; ++i) out16[i] = v[i];
    return FABHIP_OK;
}

int fabhip_spline_log_prob_tape(const fabhip_spline_flow* flow, const float* x, float* log_q, float* grad_x, int64_t B,
                                float* tape, int64_t tape_floats, void* workspace, size_t workspace_bytes,
                                fabhip_stream_t stream) {
    if (!flow || !tape || !grad_x) return FABHIP_EINVAL;
    int64_t lay[16];
    FAB_TRY(fabhip_spline_tape_layout(flow->dim, flow->n_layers, flow->hidden, B, lay));
    if (tape_floats < lay[0]) return FABHIP_ENOSPC;
    return spline_log_prob_impl(flow, x, log_q, grad_x, B, tape, workspace, workspace_bytes, (hipStream_t)stream);
}

int fabhip_spline_sample_vjp_tape(const fabhip_spline_flow* flow, const float* u, const float* eps, const float* gx, const float* gl,
                                  float* v_x, float* v_base, int64_t B, float* tape_density, float* tape_inverse,
                                  int64_t tape_floats, void* workspace, size_t workspace_bytes, fabhip_stream_t stream) {
    if (!flow || !flow->packed || !u || !eps || !v_x || !tape_density || !tape_inverse || !workspace || B < 0 || (!gx && !gl))
        return FABHIP_EINVAL;
    FAB_TRY(check_spline_shape(flow->dim, flow->n_layers, flow->hidden));
    int64_t lay[16];
    FAB_TRY(fabhip_spline_tape_layout(flow->dim, flow->n_layers, flow->hidden, B, lay));
    if (tape_floats < lay[0]) return FABHIP_ENOSPC;
    if (B == 0) return FABHIP_OK;
    if (workspace_bytes < fabhip_spline_workspace_bytes(flow->dim, flow->n_layers, flow->hidden, B, 1)) return FABHIP_ENOSPC;
    const SplineDims f = make_spline_dims(flow->dim, flow->n_layers, flow->hidden);
    hipStream_t st = (hipStream_t)stream;
    const SplineWs w = carve_spline_ws(workspace, f, (long)B, true);
    float* Z = w.Z; float* P = w.P; float* Ga = w.Ga; float* Gb = w.Gb;
    float* lq = w.dP;                                    // (the density sweep's dP scratch: here log q row sums)
    const size_t zs = (size_t)B * f.D, ps = (size_t)B * f.NFP;
    const float* pk = flow->packed;
    const dim3 wgrid((unsigned)((B + 3) / 4)), wblock(256);
    // 1. the sampler again (same kernels, same noise: the same states), every layer's output before its shift and its
    //    conditioner outputs kept: Z[l + 1] / P[l] are what the log_prob direction would recompute from x up to rounding - and
    //    the inverse of a stiff chain of splines amplifies that rounding, so the sweeps below linearise where the sample was made
    hipLaunchKernelGGL(k_spline_base_sample, wgrid, wblock, 0, st, f, pk, u, eps, Z, lq, (long)B);
    const float* zin = Z;
    for (int l = 0; l < f.L; ++l) {
        hipLaunchKernelGGL(k_spline_apply<1>, wgrid, wblock, 0, st, f, pk, l, zin, (const float*)nullptr, v_x, lq, -1.f, (long)B,
                           (float*)nullptr);
        FAB_TRY(net(f, pk, l, v_x, P + (size_t)l * ps, nullptr, nullptr, (long)B, st));
        float* out = (zin == Ga) ? Gb : Ga;
        hipLaunchKernelGGL(k_spline_apply<2>, wgrid, wblock, 0, st, f, pk, l, v_x, P + (size_t)l * ps, out, lq, -1.f, (long)B,
                           Z + (size_t)(l + 1) * zs);
        zin = out;
    }
    // 2. the log_prob direction's reverse sweep on these states (seed 1 per sample): tape_density, d log q / dx -> v_x
    const SplineTape t1 = make_spline_tape(f, (long)B, tape_density);
    hipLaunchKernelGGL(k_spline_base, wgrid, wblock, 0, st, f, pk, Z, lq, Ga, (long)B);
    float* gin = Ga;
    for (int l = 0; l < f.L; ++l) {
        float* out = (l == f.L - 1) ? v_x : (gin == Ga ? Gb : Ga);
        float* tl = tape_density + (size_t)l * t1.layer_stride;
        hipLaunchKernelGGL(k_spline_apply_bwd, wgrid, wblock, 0, st, f, pk, l, Z + (size_t)(l + 1) * zs, P + (size_t)l * ps, gin, out,
                           tl + t1.o_dP, (long)B, tl + t1.o_dU);
        FAB_TRY(net(f, pk, l, Z + (size_t)(l + 1) * zs, nullptr, tl + t1.o_dP, out, (long)B, st, t1));
        gin = out;
    }
    // 3. v at x = gx + gl * d log q / dx (in place)
    hipLaunchKernelGGL(k_spline_vjp_seed, elementwise_grid(B * f.D), dim3(256), 0, st, v_x, gx, gl, (long)B, f.D);
    // 4. v from the x side to the base side (the stage-boundary shifts and wraps have unit derivative): tape_inverse
    const SplineTape t2 = make_spline_tape(f, (long)B, tape_inverse);
    const float* vin = v_x;
    for (int l = f.L - 1; l >= 0; --l) {
        float* out = (l == 0 && v_base) ? v_base : (vin == Ga ? Gb : Ga);
        float* tl = tape_inverse + (size_t)l * t2.layer_stride;
        hipLaunchKernelGGL(k_spline_vsweep<0>, wgrid, wblock, 0, st, f, pk, l, Z + (size_t)(l + 1) * zs, P + (size_t)l * ps, vin,
                           out, tl + t2.o_dP, (long)B, (float*)nullptr);
        FAB_TRY(net(f, pk, l, Z + (size_t)(l + 1) * zs, nullptr, tl + t2.o_dP, out, (long)B, st, t2));
        hipLaunchKernelGGL(k_spline_vsweep<1>, wgrid, wblock, 0, st, f, pk, l, Z + (size_t)(l + 1) * zs, (const float*)nullptr,
                           (const float*)nullptr, out, (float*)nullptr, (long)B, tl + t2.o_dU);
        vin = out;
    }
    return check_launch();
}

int fabhip_spline_sample(const fabhip_spline_flow* flow, const float* u, const float* eps, float* x, float* log_q,
                         int64_t B, void* workspace, size_t workspace_bytes, fabhip_stream_t stream) {
    if (!flow || !flow->packed || !u || !eps || !x || !log_q || !workspace || B < 0) return FABHIP_EINVAL;
    FAB_TRY(check_spline_shape(flow->dim, flow->n_layers, flow->hidden));
    if (B == 0) return FABHIP_OK;
    if (workspace_bytes < fabhip_spline_workspace_bytes(flow->dim, flow->n_layers, flow->hidden, B, 0)) return FABHIP_ENOSPC;
    const SplineDims f = make_spline_dims(flow->dim, flow->n_layers, flow->hidden);
    hipStream_t st = (hipStream_t)stream;
    const SplineWs w = carve_spline_ws(workspace, f, (long)B, false);
    float* P = w.P;
    const size_t zs = (size_t)B * f.D;
    float* za = w.Z; float* zb = w.Z + zs; float* zc = w.Z + 2 * zs;
    const float* pk = flow->packed;
    const dim3 wgrid((unsigned)((B + 3) / 4)), wblock(256);
    hipLaunchKernelGGL(k_spline_base_sample, wgrid, wblock, 0, st, f, pk, u, eps, za, log_q, (long)B);
    for (int l = 0; l < f.L; ++l) {
        // identity coordinates through the inverse unconditional spline (zb), conditioner on them, then the rest
        hipLaunchKernelGGL(k_spline_apply<1>, wgrid, wblock, 0, st, f, pk, l, za, (const float*)nullptr, zb, log_q, -1.f, (long)B,
                           (float*)nullptr);
        FAB_TRY(net(f, pk, l, zb, P, nullptr, nullptr, (long)B, st));
        float* out = (l == f.L - 1) ? x : zc;
        hipLaunchKernelGGL(k_spline_apply<2>, wgrid, wblock, 0, st, f, pk, l, zb, P, out, log_q, -1.f, (long)B, (float*)nullptr);
        float* tmp = za; za = zc; zc = tmp;
    }
    return check_launch();
}

}  // extern "C"
