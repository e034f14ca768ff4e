// Spline coupling flow: the packed image.  One fabhip_spline_pack call turns the flow's parameter tensors into what the kernels
// read (spline_device.h: SplineDims): per layer the metadata rows, the unconditional spline parameters and the conditioner's
// weights as fp32 MFMA B-operand tiles in both orientations (k_spline_pack_layer), their bf16 images for fast mode
// (k_spline_pack_bf16) and, for hidden widths padded to 256, the stream image of spline_r8.h (k_spline_pack_r8); then the base
// distribution (k_spline_pack_base).
#include "flow_device.h"
#include "target_device.h"
#include "stream_r8.h"
#include "launch.h"
#include <stdlib.h>

#pragma clang fp contract(off)

#include "spline_device.h"

namespace fab {

__device__ __forceinline__ void sp_tile_kn(int off, int KB, int& k, int& n) {
    const int tile = off >> 8, within = off & 255;
    const int lane = within >> 2, tt = within & 3;
    const int c = tile / KB, S = tile % KB;
    k = 16 * S + 4 * (lane >> 4) + tt;
    n = 16 * c + (lane & 15);
}

__global__ __launch_bounds__(256) void k_spline_pack_layer(SplineDims f, SplineSrc s, int layer, float* __restrict__ packed) {
    float* __restrict__ dst = packed + (size_t)layer * f.layer_stride;
    const int n_id = (int)s.meta[M_CNT * 64 + 0], n_tr = (int)s.meta[M_CNT * 64 + 1], n_pf = (int)s.meta[M_CNT * 64 + 2];
    const int W = f.W, Wp = f.Wp, KBW = f.KBW, nout = n_tr * SP_NP;
    for (int off = blockIdx.x * blockDim.x + threadIdx.x; off < f.o_h; off += gridDim.x * blockDim.x) {
        float v = 0.f;
        int k, n;
        if (off < f.o_meta + SP_META_ROWS * 64) {
            v = s.meta[off - f.o_meta];
        } else if (off < f.o_meta + (SP_META_ROWS + 2) * 64) {
            const int e = off - f.o_meta - SP_META_ROWS * 64, row = e >> 6, j = e & 63;
            const int cnt = row == 0 ? n_id : n_tr;
            const float* feats = s.meta + (row == 0 ? M_IDF : M_TRF) * 64;
            v = -1.f;
            for (int i = 0; i < cnt; ++i) if ((int)feats[i] == j) v = (float)i;
        } else if (off < f.o_unc) {
            v = 0.f;
        } else if (off < f.o_pfw) {
            const int e = off - f.o_unc, i = e / SP_NP, p = e % SP_NP;
            if (i < n_id && e < SP_MD * SP_NP)
                v = p < SP_K ? s.uw[i * SP_K + p] : (p < 2 * SP_K ? s.uh[i * SP_K + p - SP_K] : s.ud[i * (SP_K + 1) + p - 2 * SP_K]);
        } else if (off < f.o_W0) {
            const int e = off - f.o_pfw;
            if (e < 2 * n_pf) v = s.pfw[e];
        } else if (off < f.o_b0) {                 // W0: B[k][n] = w0[n][k]   (k identity position, n hidden)
            sp_tile_kn(off - f.o_W0, 4, k, n);
            if (k < n_id && n < W) v = s.w0[n * n_id + k];
        } else if (off < f.o_Wa) {
            const int j = off - f.o_b0; if (j < W) v = s.b0[j];
        } else if (off < f.o_ba) {                 // Wa: B[k][n] = wa[n][k]
            sp_tile_kn(off - f.o_Wa, KBW, k, n);
            if (k < W && n < W) v = s.wa[n * W + k];
        } else if (off < f.o_Wb) {
            const int j = off - f.o_ba; if (j < W) v = s.ba[j];
        } else if (off < f.o_bb) {
            sp_tile_kn(off - f.o_Wb, KBW, k, n);
            if (k < W && n < W) v = s.wb[n * W + k];
        } else if (off < f.o_Wf) {
            const int j = off - f.o_bb; if (j < W) v = s.bb[j];
        } else if (off < f.o_bf) {                 // Wf chunk c: B[k][n] = wf[c Wp + n][k]
            const int e = off - f.o_Wf, per = 4 * f.NTWM * KBW * 256;
            const int c = e / per;
            sp_tile_kn(e % per, KBW, k, n);
            const int col = c * Wp + n;
            if (k < W && col < nout) v = s.wf[col * W + k];
        } else if (off < f.o_WfT) {
            const int j = off - f.o_bf; if (j < nout) v = s.bf[j];
        } else if (off < f.o_WbT) {                // WfT: B[k][n] = wf[k][n]   (k conditioner output, n hidden)
            sp_tile_kn(off - f.o_WfT, f.NFP / 16, k, n);
            if (k < nout && n < W) v = s.wf[k * W + n];
        } else if (off < f.o_WaT) {                // WbT: B[k][n] = wb[k][n]
            sp_tile_kn(off - f.o_WbT, KBW, k, n);
            if (k < W && n < W) v = s.wb[k * W + n];
        } else if (off < f.o_W0T) {
            sp_tile_kn(off - f.o_WaT, KBW, k, n);
            if (k < W && n < W) v = s.wa[k * W + n];
        } else {                                    // W0T: B[k][n] = w0[k][n]   (k hidden, n identity position)
            sp_tile_kn(off - f.o_W0T, KBW, k, n);
            if (k < W && n < n_id) v = s.w0[k * n_id + n];
        }
        dst[off] = v;
    }
}

__global__ void k_spline_pack_base(SplineDims f, const float* __restrict__ scale, const float* __restrict__ circ,
                                   float* __restrict__ packed) {
    const int j = threadIdx.x;
    if (j < 64) {
        packed[f.o_base + j] = j < f.D ? scale[j] : 1.f;
        packed[f.o_base + 64 + j] = j < f.D ? circ[j] : 0.f;
    }
}

// fast mode: bf16 images of the conditioner's Wp x Wp GEMM operands in v_mfma_f32_16x16x32_bf16 B-operand tiles
// (flow_device.h).  Image m of a layer, HALF = Wp^2/2 floats each, K x N:
//   0 Wa (Wp x Wp)   1 Wb   2 .. 2+NCH-1 Wf chunk c   then WfT (K = NFP: NCH HALFs, KB2T = NFP/32)   WbT   WaT
__device__ __forceinline__ unsigned sp_bf16_rne(float v) {
    unsigned u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__global__ __launch_bounds__(256) void k_spline_pack_bf16(SplineDims f, SplineSrc s, int layer, float* __restrict__ packed) {
    const int W = f.W, Wp = f.Wp, HALF = Wp * Wp / 2, n_tr = (int)s.meta[M_CNT * 64 + 1], nout = n_tr * SP_NP;
    const int total = (4 + 2 * f.NCH) * HALF;
    unsigned* __restrict__ dst = reinterpret_cast<unsigned*>(packed + (size_t)layer * f.layer_stride + f.o_h);
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        int m = e / HALF, off = e % HALF;
        int KB2T = Wp / 32;
        const bool wft = m >= 2 + f.NCH && m < 2 + 2 * f.NCH;
        if (wft) { off = e - (2 + f.NCH) * HALF; KB2T = f.NFP / 32; }      // one K = NFP image spanning NCH HALFs
        const int tile = off >> 8, lane = (off >> 2) & 63, j = 2 * (off & 3);
        const int c = tile / KB2T, S = tile % KB2T;
        const int k = 32 * S + 8 * (lane >> 4) + j, n = 16 * c + (lane & 15);
        float v[2] = {0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int kk = k + q;
            if (m == 0) { if (kk < W && n < W) v[q] = s.wa[n * W + kk]; }
            else if (m == 1) { if (kk < W && n < W) v[q] = s.wb[n * W + kk]; }
            else if (m < 2 + f.NCH) { const int col = (m - 2) * Wp + n; if (kk < W && col < nout) v[q] = s.wf[col * W + kk]; }
            else if (wft) { if (kk < nout && n < W) v[q] = s.wf[kk * W + n]; }
            else if (m == 2 + 2 * f.NCH) { if (kk < W && n < W) v[q] = s.wb[kk * W + n]; }
            else { if (kk < W && n < W) v[q] = s.wa[kk * W + n]; }
        }
        dst[e] = sp_bf16_rne(v[0]) | (sp_bf16_rne(v[1]) << 16);
    }
}

// ---- stream image (spline_r8.h) --------------------------------------------------------------------------------------------
// Layer block of the r8 image: [head | forward tiles: wave 0 .. 3 | reverse tiles: wave 0 .. 3], a wave's tiles in stream order.
__global__ __launch_bounds__(256) void k_spline_pack_r8(SplineDims f, SplineSrc s, const float* __restrict__ prev_meta,
                                                        int layer, float* __restrict__ packed) {
    const int H = s8_head_floats(f), TPL = s8_tiles_per_wave(f);
    const long total = s8_layer_floats(f);
    float* __restrict__ dst = packed + f.o_r8 + (size_t)layer * total;
    const int n_id = (int)s.meta[M_CNT * 64 + 0], n_tr = (int)s.meta[M_CNT * 64 + 1], n_pf = (int)s.meta[M_CNT * 64 + 2];
    const int W = f.W, nout = n_tr * SP_NP;
    for (long off = (long)blockIdx.x * blockDim.x + threadIdx.x; off < total; off += (long)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (off < H) {
            const int e = (int)off;
            if (e < SP_META_ROWS * 64) v = s.meta[e];
            else if (e < S8H_UNC) {                                            // M_POSID / M_POSTR (k_spline_pack_layer)
                const int q = e - SP_META_ROWS * 64, row = q >> 6, j = q & 63;
                const int cnt = row == 0 ? n_id : n_tr;
                const float* feats = s.meta + (row == 0 ? M_IDF : M_TRF) * 64;
                v = -1.f;
                for (int i = 0; i < cnt; ++i) if ((int)feats[i] == j) v = (float)i;
            } else if (e < S8H_PFW) {
                const int q = e - S8H_UNC, i = q / SP_NP, p = q % SP_NP;
                if (i < n_id && q < SP_MD * SP_NP)
                    v = p < SP_K ? s.uw[i * SP_K + p] : (p < 2 * SP_K ? s.uh[i * SP_K + p - SP_K] : s.ud[i * (SP_K + 1) + p - 2 * SP_K]);
            } else if (e < S8H_B0) { const int q = e - S8H_PFW; if (q < 2 * n_pf) v = s.pfw[q]; }
            else if (e < S8H_BA) { const int j = e - S8H_B0; if (j < W) v = s.b0[j]; }
            else if (e < S8H_BB) { const int j = e - S8H_BA; if (j < W) v = s.ba[j]; }
            else if (e < S8H_NXT) { const int j = e - S8H_BB; if (j < W) v = s.bb[j]; }
            else if (e < S8H_BF) {                                             // pre-shift of the NEXT stage (layer - 1): shift | on
                const int q = e - S8H_NXT;
                if (prev_meta) v = prev_meta[(q < 64 ? M_PRESH : M_PREON) * 64 + (q & 63)];
            } else { const int j = e - S8H_BF; if (j < nout) v = s.bf[j]; }
        } else {
            const long e = off - H;
            const int kk = (int)(e & 3), lane = (int)((e >> 2) & 63);
            const long tl = e >> 8;
            const int tile = (int)(tl % TPL), wave = (int)((tl / TPL) % NWAVE), dir = (int)(tl / ((long)TPL * NWAVE));
            const int n = 64 * wave + lane;
            // round 5 (f.r8_trim): the stream without zero tiles - W0 as K0Q = 4 k-quads, WfT as KFQ = 100, W0T as 4 dense tiles
            const int K0Q = f.r8_trim ? 4 : 16, KFQ = f.r8_trim ? 100 : 64 * f.NCH;
            if (dir == 0) {
                if (tile < K0Q) {                                              // W0: B[k][n] = w0[n][k]
                    const int k = 4 * tile + kk;
                    if (k < n_id && n < W) v = s.w0[n * n_id + k];
                } else if (tile < K0Q + 64 * (2 + f.NCH)) {
                    const int t2 = tile - K0Q, m = t2 >> 6, k = 4 * (t2 & 63) + kk;
                    if (m == 0) { if (k < W && n < W) v = s.wa[n * W + k]; }
                    else if (m == 1) { if (k < W && n < W) v = s.wb[n * W + k]; }
                    else { const int col = (m - 2) * 256 + n; if (k < W && col < nout) v = s.wf[col * W + k]; }
                }
            } else {
                if (tile < KFQ) {                                              // WfT: B[k][n] = wf[k][n]
                    const int k = 4 * tile + kk;
                    if (k < nout && n < W) v = s.wf[k * W + n];
                } else {
                    const int t2 = tile - KFQ;
                    if (t2 < 64) { const int k = 4 * t2 + kk; if (k < W && n < W) v = s.wb[k * W + n]; }
                    else if (t2 < 128) { const int k = 4 * (t2 - 64) + kk; if (k < W && n < W) v = s.wa[k * W + n]; }
                    else if (!f.r8_trim) {                                     // W0T, K split over the waves: B[k][i] = w0[k][i]
                        if (t2 < 144) {
                            const int k = 64 * wave + 4 * (t2 - 128) + kk;
                            if (k < W && lane < n_id) v = s.w0[k * n_id + lane];
                        }
                    } else if (t2 < 132) {                                     // ... as dense tiles: 4 k-quads x 16 identity features
                        const int k = 64 * wave + 4 * (4 * (t2 - 128) + (lane >> 4)) + kk, c = lane & 15;
                        if (k < W && c < n_id) v = s.w0[k * n_id + c];
                    }
                }
            }
        }
        dst[off] = v;
    }
}

}  // namespace fab

using namespace fab;

extern "C" {

int64_t fabhip_spline_packed_floats(int32_t dim, int32_t n_layers, int32_t hidden) {
    if (check_spline_shape(dim, n_layers, hidden) != FABHIP_OK) return -1;
    return (int64_t)make_spline_dims(dim, n_layers, hidden).total;
}

int fabhip_spline_pack(const fabhip_spline_params* p, float* packed, fabhip_stream_t stream) {
    if (!p || !packed || !p->base_scale || !p->base_circ) return FABHIP_EINVAL;
    FAB_TRY(check_spline_shape(p->dim, p->n_layers, p->hidden));
    const SplineDims f = make_spline_dims(p->dim, p->n_layers, p->hidden);
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l < f.L; ++l) {
        if (!p->meta[l] || !p->w0[l] || !p->b0[l] || !p->wa[l] || !p->ba[l] || !p->wb[l] || !p->bb[l] || !p->wf[l] ||
            !p->bf[l] || !p->uw[l] || !p->uh[l] || !p->ud[l])
            return FABHIP_EINVAL;
        const SplineSrc s{p->meta[l], p->w0[l], p->b0[l], p->wa[l], p->ba[l], p->wb[l], p->bb[l], p->wf[l], p->bf[l],
                          p->pfw[l], p->uw[l], p->uh[l], p->ud[l]};
        hipLaunchKernelGGL(k_spline_pack_layer, dim3(ceil_div(f.o_h, 256 * 8)), dim3(256), 0, st, f, s, l, packed);
        hipLaunchKernelGGL(k_spline_pack_bf16, dim3(ceil_div((4 + 2 * f.NCH) * (f.Wp * f.Wp / 2), 256 * 8)), dim3(256), 0, st,
                           f, s, l, packed);
        if (f.o_r8)
            hipLaunchKernelGGL(k_spline_pack_r8, dim3(ceil_div(f.r8_layer, 256 * 8)), dim3(256), 0, st, f, s,
                               l > 0 ? p->meta[l - 1] : (const float*)nullptr, l, packed);
    }
    hipLaunchKernelGGL(k_spline_pack_base, dim3(1), dim3(64), 0, st, f, p->base_scale, p->base_circ, packed);
    return check_launch();
}

}  // extern "C"
