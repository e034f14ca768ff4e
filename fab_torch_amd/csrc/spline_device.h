// Spline coupling flow, device side shared by the spline units (spline_pack.hip, spline_tile16.hip, spline_stream.hip): the constants and the metadata rows, the packed image's layout (SplineDims, the head block of the
// stream image), the training tape's layout, the conditioner's LDS plan with its GEMM / tile helpers on 16-chain tiles, and
// the rational-quadratic spline element functions every spline kernel evaluates (one definition: the kernels stay
// bit-compatible).  Included behind the unit's `#pragma clang fp contract(off)`.
#pragma once
#include "flow_device.h"
#include "launch.h"

namespace fab {

constexpr int SP_K = 8;                 // bins
constexpr int SP_NP = 3 * SP_K + 1;     // parameters per coordinate: K widths, K heights, K + 1 knot derivatives
constexpr int SP_MD = 64;               // max dim
constexpr int SP_META_ROWS = 12;        // per-layer metadata rows of 64 floats (see fabhip.h)
constexpr float SP_MIN_W = 1e-3f, SP_MIN_H = 1e-3f, SP_MIN_D = 1e-3f;

enum { M_IDF = 0, M_TRF = 1, M_CIRC = 2, M_TB = 3, M_PFON = 4, M_PFS = 5, M_PFK = 6, M_PRESH = 7, M_PREON = 8,
       M_POSTSH = 9, M_POSTON = 10, M_CNT = 11,
       M_POSID = 12, M_POSTR = 13 };      // derived at pack time: position of coordinate j among the identity / transformed
                                          // features of the layer (-1: not one), so the element-wise kernels need no search

// head block of a layer in the r8 image (floats); the first three regions sit where SplineDims puts them in a layer image
constexpr int S8H_META = 0, S8H_UNC = (SP_META_ROWS + 2) * 64, S8H_PFW = S8H_UNC + 1664, S8H_B0 = S8H_PFW + 128,
              S8H_BA = S8H_B0 + 256, S8H_BB = S8H_BA + 256, S8H_NXT = S8H_BB + 256, S8H_BF = S8H_NXT + 128;

struct SplineDims {
    int D, L, W, Wp, NTWM, KBW;          // hidden width, padded to 64 * tiles-per-wave
    int n_tr_max, NCH, NFP;              // chunks of Wp conditioner outputs: NFP = NCH * Wp >= n_tr_max * SP_NP
    int o_meta, o_unc, o_pfw, o_W0, o_b0, o_Wa, o_ba, o_Wb, o_bb, o_Wf, o_bf, o_WfT, o_WbT, o_WaT, o_W0T;
    int o_h;                             // fast mode: bf16 images [Wa | Wb | Wf (NCH chunks) | WfT | WbT | WaT], Wp^2/2 floats per Wp x Wp
    int layer_stride, o_base, total;
    // 8-chain-tile image (spline_r8.h; Wp == 256 only, else o_r8 == 0): per layer [head | forward tiles | reverse tiles]
    int o_r8, r8_head, r8_tpl, r8_layer; // head floats, 1-KiB tiles per wave and direction, floats per layer
    int r8_trim;                         // round 5: the r8 stream without its zero tiles (D <= 32 with two output chunks: <= 16 identity
                                         // features -> W0 is 4 k-quads, not 16; <= 400 conditioner outputs -> WfT is 100 k-quads, not
                                         // 128; W0T as 4 dense tiles, not 16): 260 + 232 instead of 272 + 272 tiles per wave and layer
};

FAB_HD SplineDims make_spline_dims(int D, int L, int W) {
    SplineDims f;
    f.D = D; f.L = L; f.W = W;
    f.NTWM = ntw_variant(W); f.Wp = 64 * f.NTWM; f.KBW = f.Wp / 16;
    f.n_tr_max = (D + 1) / 2;
    f.NCH = ceil_div(f.n_tr_max * SP_NP, f.Wp);
    f.NFP = f.NCH * f.Wp;
    int o = 0;
    f.o_meta = o; o += (SP_META_ROWS + 2) * 64;
    f.o_unc = o; o += SP_MD * SP_NP + 32;                 // [64][25] (+ pad to a multiple of 64 floats below)
    o = (o + 63) & ~63;
    f.o_pfw = o; o += 2 * SP_MD;                           // [64][2] periodic-feature weights
    const int T = f.KBW * 256;                             // floats per column-tile strip of K = Wp
    f.o_W0 = o; o += 4 * (4 * f.NTWM) * 256;              // K = 64 (identity coordinates, padded), N = Wp
    f.o_b0 = o; o += f.Wp;
    f.o_Wa = o; o += (4 * f.NTWM) * T;
    f.o_ba = o; o += f.Wp;
    f.o_Wb = o; o += (4 * f.NTWM) * T;
    f.o_bb = o; o += f.Wp;
    f.o_Wf = o; o += f.NCH * (4 * f.NTWM) * T;            // NCH chunks of [Wp x Wp]
    f.o_bf = o; o += f.NFP;
    f.o_WfT = o; o += (4 * f.NTWM) * (f.NFP / 16) * 256;  // K = NFP, N = Wp
    f.o_WbT = o; o += (4 * f.NTWM) * T;
    f.o_WaT = o; o += (4 * f.NTWM) * T;
    f.o_W0T = o; o += 4 * T;                               // K = Wp, N = 64
    f.o_h = o; o += (4 + 2 * f.NCH) * (f.Wp * f.Wp / 2);
    f.layer_stride = o;
    f.o_base = L * f.layer_stride;                         // scale[64], circ[64]
    f.total = f.o_base + 128;
    f.o_r8 = 0;
    f.r8_head = S8H_BF + f.NFP;
    f.r8_tpl = 16 + 64 * (2 + f.NCH);
    f.r8_trim = (f.NCH == 2 && (D + 1) / 2 <= 16) ? 1 : 0;
    f.r8_layer = f.r8_head + 2 * NWAVE * f.r8_tpl * 256;
    if (f.NTWM == 4) {
        f.o_r8 = (f.total + 255) & ~255;
        f.total = f.o_r8 + L * f.r8_layer;
    }
    return f;
}

static inline int check_spline_shape(int D, int L, int W) {
    if (D < 2 || L < 1 || W < 1) return FABHIP_EINVAL;
    if (D > SP_MD || L > FABHIP_MAX_LAYERS || W > 256) return FABHIP_ENOTSUP;       // NTWM in {1, 2, 4}
    return FABHIP_OK;
}

// Training tape of one log_prob call (fabhip_spline_log_prob_tape): per coupling layer, row-major [B][width] matrices
// of the conditioner's activations and of the reverse sweep's cotangents (seed 1 per sample).  The weight gradients
// are sum_b c_b (cotangent row)^T (activation row): GEMMs over these matrices, done by the caller (rocBLAS through
// torch.mm in fab_torch_amd/spline_flow.py) with the per-sample coefficient c_b folded into the cotangent rows.
struct SplineTape {
    float* base;                          // nullptr: no tape
    long o_XI, o_A0, o_dA0;               // [B][64]: raw identity coordinates, after the periodic features, cotangent of A0
    long o_R0, o_R1, o_H1;                // [B][Wp]: relu(h0), relu(t), h1
    long o_dH1, o_dT, o_dH0;              // [B][Wp]: cotangents of h1, of t (masked), of h0
    long o_dP;                            // [B][NFP]: cotangent of the conditioner output
    long o_dU;                            // [B][64 * 25]: cotangent of the unconditional parameters per identity position
    long layer_stride;
};

static inline SplineTape make_spline_tape(const SplineDims& f, long B, float* base) {
    SplineTape t;
    t.base = base;
    long o = 0;
    t.o_XI = o; o += B * 64; t.o_A0 = o; o += B * 64; t.o_dA0 = o; o += B * 64;
    t.o_R0 = o; o += B * f.Wp; t.o_R1 = o; o += B * f.Wp; t.o_H1 = o; o += B * f.Wp;
    t.o_dH1 = o; o += B * f.Wp; t.o_dT = o; o += B * f.Wp; t.o_dH0 = o; o += B * f.Wp;
    t.o_dP = o; o += B * f.NFP;
    t.o_dU = o; o += B * (long)(SP_MD * SP_NP);
    t.layer_stride = o;
    return t;
}

// the parameter tensors of one layer as fabhip_spline_pack receives them (spline_pack.hip)
struct SplineSrc {
    const float *meta, *w0, *b0, *wa, *ba, *wb, *bb, *wf, *bf, *pfw, *uw, *uh, *ud;
};

// the stream image of a layer (spline_r8.h): [head | forward tiles: wave 0 .. 3 | reverse tiles: wave 0 .. 3]
FAB_HD int s8_head_floats(const SplineDims& f) { return f.r8_head; }                      // S8H_BF + NFP: a multiple of 128
FAB_HD int s8_tiles_per_wave(const SplineDims& f) { return f.r8_tpl; }                    // per layer and direction: 16 + 64 (2 + NCH)
FAB_HD long s8_layer_floats(const SplineDims& f) { return f.r8_layer; }

// ------------------------------------------------------------------------------------------------
// conditioner (ResidualNet) on a 16-chain tile
// ------------------------------------------------------------------------------------------------
struct NetLds {
    int AS, WS, PS;                       // leading dims: identity inputs (64 + 4), hidden (Wp + 4), dparams (NFP + 4)
    int o_A0, o_H0, o_T, o_X1, o_X2, o_DP, o_PART, total;
    int o_ZT, o_GT;                       // persistent kernel: state tile and cotangent tile [16][64]
};
// persist: the one-launch density kernel (k_spline_logprob): + state / cotangent tiles; its conditioner output P lives
// in the DP region (the reverse sweep turns it into dP in place)
FAB_HD NetLds make_net_lds(const SplineDims& f, bool bwd, bool persist = false) {
    NetLds l;
    l.AS = 64 + 4; l.WS = f.Wp + 4; l.PS = f.NFP + 4;
    int o = 0;
    l.o_A0 = o; o += ROWS * l.AS;
    l.o_H0 = o; o += ROWS * l.WS;
    l.o_T = o; o += ROWS * l.WS;
    l.o_X1 = o; o += ROWS * l.WS;
    l.o_X2 = o; o += ROWS * l.WS;
    l.o_DP = o; if (bwd || persist) o += ROWS * l.PS;
    l.o_PART = o; if (bwd) o += NWAVE * ROWS * l.AS;
    l.o_ZT = o; if (persist) o += ROWS * 64;
    l.o_GT = o; if (persist) o += ROWS * 64;
    l.total = (o + 3) & ~3;
    return l;
}

// plain GEMM on the tile: acc[i] = A[16 x 16 KB] @ B[:, tile wave + 4 i] (+ bias)
template <int NTWM, int DEPTH, bool BIAS>
__device__ __forceinline__ void sp_gemm(const float* A, int lda, int KB, const float4* Bp, const float* bias, const Tid& t,
                                        f32x4 (&acc)[NTWM]) {
    WRing<NTWM, DEPTH> w;
    if (!BIAS) {
#pragma unroll
        for (int i = 0; i < NTWM; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    ring_issue<NTWM, DEPTH, BIAS>(w, Bp, KB, bias, t);
    ring_run<NTWM, DEPTH, false, BIAS>(w, A, lda, 0, KB, Bp, t, acc);
}

// fast-mode twin of sp_gemm for the Wp x Wp operands: image `m` of the layer's bf16 block (see k_spline_pack_bf16)
template <int NTWM, bool BIAS>
__device__ __forceinline__ void sp_gemm_bf16(const SplineDims& f, const float* A, int lda, const float* __restrict__ Lp, int m,
                                             const float* bias, const Tid& t, f32x4 (&acc)[NTWM]) {
#pragma unroll
    for (int i = 0; i < NTWM; ++i) {
        const float bv = BIAS ? bias[16 * (t.wave + 4 * i) + t.n] : 0.f;
        acc[i] = (f32x4){bv, bv, bv, bv};
    }
    const uint4* Bh = reinterpret_cast<const uint4*>(Lp + f.o_h + (size_t)m * (f.Wp * f.Wp / 2));
    gemm_bf16_slice<NTWM>(A, lda, Bh, f.Wp / 32, 0, t, acc);
}

// identity coordinates of the tile with their periodic features -> A0 (columns >= n_id zero); returns nothing
__device__ __forceinline__ void sp_load_identity(const SplineDims& f, const float* __restrict__ Lp, const float* __restrict__ Z,
                                                 long row0, long B, float* A0, int AS, const Tid& t) {
    const float* meta = Lp + f.o_meta;
    const int n_id = (int)meta[M_CNT * 64];
    for (int e = t.tid; e < ROWS * AS; e += NTHREADS) {
        const int r = e / AS, i = e % AS;
        const long g = row0 + r;
        float v = 0.f;
        if (i < n_id && g < B) {
            const int feat = (int)meta[M_IDF * 64 + i];
            v = Z[g * f.D + feat];
            if (meta[M_PFON * 64 + i] != 0.f) {
                const int k = (int)meta[M_PFK * 64 + i];
                const float s = meta[M_PFS * 64 + i];
                v = Lp[f.o_pfw + 2 * k] * sinf(s * v) + Lp[f.o_pfw + 2 * k + 1] * cosf(s * v);
            }
        }
        A0[e] = v;
    }
}

// rows row0 .. row0+15 of a row-major [B][width] matrix (width % 4 == 0, 16-byte aligned rows) -> LDS tile [16][ldd]:
// one wave per row (4 rows each), float4 per lane, no index division (the element-wise version of this load cost 27 %
// of the reverse sweep)
__device__ __forceinline__ void sp_tile_load4(float* dst, int ldd, const float* __restrict__ src, long lds_src, int width,
                                              long row0, long B, const Tid& t) {
    for (int r = t.wave; r < ROWS; r += NWAVE) {
        const long g = row0 + r;
        for (int c4 = t.lane; 4 * c4 < width; c4 += 64) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (g < B) v = *reinterpret_cast<const float4*>(src + g * lds_src + 4 * c4);
            *reinterpret_cast<float4*>(dst + r * ldd + 4 * c4) = v;
        }
    }
}

// the reverse: LDS tile [16][lds_src] -> rows row0 .. of a row-major [B][ldd] matrix, float4 per lane
__device__ __forceinline__ void sp_tile_store4(float* __restrict__ dst, long ldd, const float* src, int lds_src, int width,
                                               long row0, long B, const Tid& t) {
    for (int r = t.wave; r < ROWS; r += NWAVE) {
        const long g = row0 + r;
        if (g < B)
            for (int c4 = t.lane; 4 * c4 < width; c4 += 64)
                *reinterpret_cast<float4*>(dst + g * ldd + 4 * c4) = *reinterpret_cast<const float4*>(src + r * lds_src + 4 * c4);
    }
}

// tape: rows of an LDS tile [16][ld] (first `width` columns) -> dst [B][width]
__device__ __forceinline__ void sp_tape_rows(float* __restrict__ dst, int width, const float* src, int ld, long row0, long B,
                                             const Tid& t) {
    for (int e = t.tid; e < ROWS * width; e += NTHREADS) {
        const int r = e / width, c = e % width;
        if (row0 + r < B) dst[(row0 + r) * width + c] = src[r * ld + c];
    }
}

// h0 = A0 W0 + b0 (kept raw in H0), t = relu(h0) Wa + ba (kept raw in T), h1 = h0 + relu(t) Wb + bb -> X1
// `bits` (nullable, the one-launch kernel): the ReLU decisions of h0 and t as one 64-bit ballot per (wave, tile, r) -
// 2 * 4 * NTWM * 4 words per 16-chain tile - for the reverse sweep (which then needs no activations at all).
// `act` (nullable): relu(h0) | relu(t) of the tile's rows are kept ([B][2 Wp], rows row0..) for k_spline_net_bwd, which
// then only needs their signs (the ReLU decisions) and skips this recomputation.
template <int NTWM, bool FAST = false>
__device__ __forceinline__ void sp_net_hidden(const SplineDims& f, const NetLds& l, const float* __restrict__ Lp, float* lds,
                                              const Tid& t, float* __restrict__ act = nullptr, long row0 = 0, long B = 0,
                                              unsigned long long* __restrict__ bits = nullptr) {
    constexpr int DW = depth_w<NTWM>();
    float* A0 = lds + l.o_A0; float* H0 = lds + l.o_H0; float* T = lds + l.o_T;
    float* X1 = lds + l.o_X1; float* X2 = lds + l.o_X2;
    f32x4 acc[NTWM];
    sp_gemm<NTWM, 2, true>(A0, l.AS, 4, reinterpret_cast<const float4*>(Lp + f.o_W0), Lp + f.o_b0, t, acc);
#pragma unroll
    for (int i = 0; i < NTWM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (4 * t.q + r) * l.WS + 16 * (t.wave + 4 * i) + t.n;
            H0[o] = acc[i][r];
            X2[o] = acc[i][r] > 0.f ? acc[i][r] : 0.f;
            if (act && row0 + 4 * t.q + r < B)
                act[(row0 + 4 * t.q + r) * (2 * f.Wp) + 16 * (t.wave + 4 * i) + t.n] = X2[o];
            if (bits) {                                  // ReLU decisions of (rows 4q + r, tile wave + 4 i): one word per wave
                const unsigned long long m = __ballot(acc[i][r] > 0.f);
                if (t.lane == 0) bits[((0 * NWAVE + t.wave) * NTWM + i) * 4 + r] = m;
            }
        }
    __syncthreads();
    if constexpr (FAST) sp_gemm_bf16<NTWM, true>(f, X2, l.WS, Lp, 0, Lp + f.o_ba, t, acc);
    else sp_gemm<NTWM, DW, true>(X2, l.WS, f.KBW, reinterpret_cast<const float4*>(Lp + f.o_Wa), Lp + f.o_ba, t, acc);
#pragma unroll
    for (int i = 0; i < NTWM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (4 * t.q + r) * l.WS + 16 * (t.wave + 4 * i) + t.n;
            T[o] = acc[i][r];
            X1[o] = acc[i][r] > 0.f ? acc[i][r] : 0.f;
            if (act && row0 + 4 * t.q + r < B)
                act[(row0 + 4 * t.q + r) * (2 * f.Wp) + f.Wp + 16 * (t.wave + 4 * i) + t.n] = X1[o];
            if (bits) {
                const unsigned long long m = __ballot(acc[i][r] > 0.f);
                if (t.lane == 0) bits[((1 * NWAVE + t.wave) * NTWM + i) * 4 + r] = m;
            }
        }
    __syncthreads();
    if constexpr (FAST) sp_gemm_bf16<NTWM, true>(f, X1, l.WS, Lp, 1, Lp + f.o_bb, t, acc);
    else sp_gemm<NTWM, DW, true>(X1, l.WS, f.KBW, reinterpret_cast<const float4*>(Lp + f.o_Wb), Lp + f.o_bb, t, acc);
    __syncthreads();                                   // everybody is done reading X1 (relu(t)) before it is overwritten
#pragma unroll
    for (int i = 0; i < NTWM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (4 * t.q + r) * l.WS + 16 * (t.wave + 4 * i) + t.n;
            X1[o] = H0[o] + acc[i][r];
        }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// rational-quadratic spline (Durkan et al. 2019, eqs. 4-8; nflows / normflows rational_quadratic_spline)
// ------------------------------------------------------------------------------------------------
// The spline arithmetic below uses the hardware transcendental forms (__expf = v_exp_f32 on a scaled argument, __logf =
// v_log_f32 scaled: ~1-2 ulp) - the dependent exp / log chains of a coordinate are what bounds the element-wise part
// of the kernels, and 2e-7 relative is far inside the 1e-4 parity bar (softplus keeps log1pf where exp(u) is tiny).
// Round 5: quotients by a shared denominator are products with its hardware reciprocal (v_rcp_f32, 1 ulp; every
// denominator here is a softmax sum >= 1, a bin width / height >= 2 tb MIN, or a positive rational-quadratic term): an IEEE
// fp32 division is ~10 dependent instructions, a coordinate had 17 in the forward and 29 in the reverse pass - 2 + 2 and 2 + 6
// reciprocals now.  Shared by every spline kernel (16- / 8-chain tiles, sampling, tape), so they stay bit-compatible.
__device__ __forceinline__ float sp_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
struct Rqs {
    float cw[SP_K + 1], ch[SP_K + 1];                    // knot positions / values
    float ud[SP_K + 1];                                  // effective unnormalised knot derivatives (end knots fixed / tied)
    float pw[SP_K], ph[SP_K];                            // softmax probabilities (backward)
    bool circ;
};
// derivative min + softplus(u) of knot j and (backward) its d/du = sigmoid(u), 0 for a fixed end knot - evaluated only
// for the two knots of the bin that holds x (9 softplus + 9 sigmoid per coordinate otherwise)
__device__ __forceinline__ float sp_softplus(float x);
__device__ __forceinline__ void rqs_knot_pair(const Rqs& s, int b, float& d0, float& d1, float* sg0, float* sg1) {
    float u0 = s.ud[0], u1 = s.ud[1];
#pragma unroll
    for (int j = 1; j < SP_K; ++j)
        if (j == b) { u0 = s.ud[j]; u1 = s.ud[j + 1]; }
    d0 = SP_MIN_D + sp_softplus(u0);
    d1 = SP_MIN_D + sp_softplus(u1);
    if (sg0) {
        const bool f0 = !s.circ && b == 0, f1 = !s.circ && b == SP_K - 1;
        *sg0 = f0 ? 0.f : sp_rcp(1.f + __expf(-u0));
        *sg1 = f1 ? 0.f : sp_rcp(1.f + __expf(-u1));
    }
}

__device__ __forceinline__ float sp_softplus(float x) { return x > 20.f ? x : (x < -5.f ? log1pf(expf(x)) : __logf(1.f + __expf(x))); }

// p[0..K) widths, [K..2K) heights (both already divided by sqrt(hidden) when conditional), [2K..3K] derivatives
__device__ __forceinline__ void rqs_setup(const float* p, bool circ, float tb, Rqs& s) {
    float mw = p[0], mh = p[SP_K];
#pragma unroll
    for (int j = 1; j < SP_K; ++j) { mw = fmaxf(mw, p[j]); mh = fmaxf(mh, p[SP_K + j]); }
    float sw = 0.f, sh = 0.f;
#pragma unroll
    for (int j = 0; j < SP_K; ++j) { s.pw[j] = __expf(p[j] - mw); sw += s.pw[j]; s.ph[j] = __expf(p[SP_K + j] - mh); sh += s.ph[j]; }
    float cw = 0.f, chh = 0.f;
    s.cw[0] = -tb; s.ch[0] = -tb;
    const float isw = sp_rcp(sw), ish = sp_rcp(sh);
#pragma unroll
    for (int j = 0; j < SP_K; ++j) {
        s.pw[j] = s.pw[j] * isw; s.ph[j] = s.ph[j] * ish;
        cw += SP_MIN_W + (1.f - SP_MIN_W * SP_K) * s.pw[j];
        chh += SP_MIN_H + (1.f - SP_MIN_H * SP_K) * s.ph[j];
        s.cw[j + 1] = (2.f * tb) * cw + (-tb);
        s.ch[j + 1] = (2.f * tb) * chh + (-tb);
    }
    s.cw[SP_K] = tb; s.ch[SP_K] = tb;
    const float cst = __logf(__expf(1.f - SP_MIN_D) - 1.f);
    s.circ = circ;
#pragma unroll
    for (int j = 0; j <= SP_K; ++j) {
        float u = p[2 * SP_K + j];
        if (!circ && (j == 0 || j == SP_K)) u = cst;
        if (circ && j == SP_K) u = p[2 * SP_K];
        s.ud[j] = u;
    }
}

__device__ __forceinline__ int rqs_bin(const float* knots, float x) {
    int b = 0;
#pragma unroll
    for (int j = 1; j < SP_K; ++j) b += (x >= knots[j]) ? 1 : 0;
    return b;                                             // clamp(sum(x >= knots (last + eps)) - 1, 0, K - 1), x in [-B, B]
}

// y = f(x), logabsdet; identity outside [-tb, tb]
__device__ __forceinline__ void rqs_forward(const Rqs& s, float x, float tb, float& y, float& ld) {
    if (!(x >= -tb && x <= tb)) { y = x; ld = 0.f; return; }
    const int b = rqs_bin(s.cw, x);
    float xk = 0.f, w = 1.f, yk = 0.f, h = 1.f, d0, d1;
#pragma unroll
    for (int j = 0; j < SP_K; ++j)
        if (j == b) { xk = s.cw[j]; w = s.cw[j + 1] - s.cw[j]; yk = s.ch[j]; h = s.ch[j + 1] - s.ch[j]; }
    rqs_knot_pair(s, b, d0, d1, nullptr, nullptr);
    const float iw = sp_rcp(w);
    const float th = (x - xk) * iw, t1 = th * (1.f - th), dl = h * iw;
    const float num = h * (dl * (th * th) + d0 * t1);
    const float den = dl + (d0 + d1 - 2.f * dl) * t1;
    y = yk + num * sp_rcp(den);
    const float dn = (dl * dl) * (d1 * (th * th) + 2.f * dl * t1 + d0 * ((1.f - th) * (1.f - th)));
    ld = __logf(dn) - 2.f * __logf(den);
}

// x = f^-1(y), logabsdet of the INVERSE map
__device__ __forceinline__ void rqs_inverse(const Rqs& s, float y, float tb, float& x, float& ld) {
    if (!(y >= -tb && y <= tb)) { x = y; ld = 0.f; return; }
    const int b = rqs_bin(s.ch, y);
    float xk = 0.f, w = 1.f, yk = 0.f, h = 1.f, d0, d1;
#pragma unroll
    for (int j = 0; j < SP_K; ++j)
        if (j == b) { xk = s.cw[j]; w = s.cw[j + 1] - s.cw[j]; yk = s.ch[j]; h = s.ch[j + 1] - s.ch[j]; }
    rqs_knot_pair(s, b, d0, d1, nullptr, nullptr);
    const float dl = h * sp_rcp(w), dy = y - yk, A = d0 + d1 - 2.f * dl;
    const float a = dy * A + h * (dl - d0);
    const float bq = h * d0 - dy * A;
    const float c = -dl * dy;
    const float disc = bq * bq - 4.f * a * c;
    // (on a knot whose derivative is near SP_MIN_D the discriminant is (h d)^2, the difference of two terms ~ (2 h dl)^2: it rounds
    // below zero there - the sample was NaN - and the bin fraction leaves [0, 1] by up to d / (2 dl), enough to turn `dn` below
    // negative - log q was NaN beside a finite x).  fmaxf / fminf return the other operand for a NaN: a NaN root (NaN parameters)
    // becomes 0 here, and the NaN still reaches x and ld through w, xk and dl
    const float root = fminf(fmaxf((2.f * c) * sp_rcp(-bq - sqrtf(fmaxf(disc, 0.f))), 0.f), 1.f);
    x = root * w + xk;
    const float t1 = root * (1.f - root);
    const float den = dl + A * t1;
    const float dn = (dl * dl) * (d1 * (root * root) + 2.f * dl * t1 + d0 * ((1.f - root) * (1.f - root)));
    ld = -(__logf(dn) - 2.f * __logf(den));
}

// reverse mode of rqs_forward with cotangents (gy, 1 on logabsdet): returns d/dx and, if dp != nullptr, the cotangents
// of the 3K+1 unnormalised parameters (scaled by `wh_scale` for widths / heights).  LD = false: cotangents (gy, 0) - the map
// alone, without its log-derivative (k_spline_vsweep)
template <bool LD = true>
__device__ __forceinline__ float rqs_backward(const Rqs& s, const float* p, bool circ, float x, float tb, float gy,
                                              float wh_scale, float* dp) {
    if (dp) {
#pragma unroll
        for (int j = 0; j < SP_NP; ++j) dp[j] = 0.f;
    }
    if (!(x >= -tb && x <= tb)) return gy;
    const int b = rqs_bin(s.cw, x);
    float xk = 0.f, w = 1.f, h = 1.f, d0, d1, sg0 = 0.f, sg1 = 0.f;
#pragma unroll
    for (int j = 0; j < SP_K; ++j)
        if (j == b) { xk = s.cw[j]; w = s.cw[j + 1] - s.cw[j]; h = s.ch[j + 1] - s.ch[j]; }
    rqs_knot_pair(s, b, d0, d1, dp ? &sg0 : nullptr, dp ? &sg1 : nullptr);
    const float iw = sp_rcp(w), ih = sp_rcp(h);
    const float th = (x - xk) * iw, t1 = th * (1.f - th), dl = h * iw, A = d0 + d1 - 2.f * dl;
    const float num = h * (dl * (th * th) + d0 * t1);
    const float den = dl + A * t1;
    const float e = d1 * (th * th) + 2.f * dl * t1 + d0 * ((1.f - th) * (1.f - th));
    const float iden = sp_rcp(den);
    const float nb = gy * iden;                                    // cotangent of num
    const float db = LD ? -gy * num * (iden * iden) - 2.f * iden : -gy * num * (iden * iden);       // of den
    const float eb = LD ? sp_rcp(e) : 0.f;                         // of e
    const float sb = (LD ? 2.f * (w * ih) : 0.f) + eb * 2.f * t1 + db * (1.f - 2.f * t1) + nb * h * (th * th);   // (2 / dl = 2 w / h)
    const float t1b = eb * 2.f * dl + db * A + nb * h * d0;
    const float d0b = eb * ((1.f - th) * (1.f - th)) + db * t1 + nb * h * t1;
    const float d1b = eb * (th * th) + db * t1;
    const float thb = eb * (2.f * d1 * th - 2.f * d0 * (1.f - th)) + nb * 2.f * h * dl * th + t1b * (1.f - 2.f * th);
    const float hb = nb * (num * ih) + sb * iw;
    const float wb = -sb * h * (iw * iw) - thb * th * iw;
    const float xb = thb * iw;
    if (dp) {
        // knots: W_b += -xb - wb, W_{b+1} += wb ; H_b += gy - hb, H_{b+1} += hb ; D_b += d0b, D_{b+1} += d1b
        const float cWb = -xb - wb, cW1 = wb, cHb = gy - hb, cH1 = hb;
        // W_j = -tb + 2 tb (j MIN + (1 - K MIN) P_j), P_j = sum_{i<j} p_i  ->  d uw_m = c p_m sum_j cW_j (1[m < j] - P_j)
        const float cw_ = 2.f * tb * (1.f - SP_MIN_W * SP_K), chh = 2.f * tb * (1.f - SP_MIN_H * SP_K);
        float Pw = 0.f, Ph = 0.f, Pwb = 0.f, Pw1 = 0.f, Phb = 0.f, Ph1 = 0.f;
#pragma unroll
        for (int j = 0; j <= SP_K; ++j) {
            if (j == b) { Pwb = Pw; Phb = Ph; }
            if (j == b + 1) { Pw1 = Pw; Ph1 = Ph; }
            if (j < SP_K) { Pw += s.pw[j]; Ph += s.ph[j]; }
        }
        const bool fb = b >= 1, f1 = b + 1 <= SP_K - 1;           // the end knots W_0, W_K are fixed
#pragma unroll
        for (int m = 0; m < SP_K; ++m) {
            float aw = 0.f, ah = 0.f;
            if (fb) { aw += cWb * ((m < b ? 1.f : 0.f) - Pwb); ah += cHb * ((m < b ? 1.f : 0.f) - Phb); }
            if (f1) { aw += cW1 * ((m < b + 1 ? 1.f : 0.f) - Pw1); ah += cH1 * ((m < b + 1 ? 1.f : 0.f) - Ph1); }
            dp[m] = cw_ * s.pw[m] * aw * wh_scale;
            dp[SP_K + m] = chh * s.ph[m] * ah * wh_scale;
        }
#pragma unroll
        for (int j = 0; j <= SP_K; ++j) {
            float g = 0.f;
            if (j == b) g += d0b * sg0;
            if (j == b + 1) g += d1b * sg1;
            if (circ && j == SP_K) { dp[2 * SP_K] += g; g = 0.f; }            // last knot tied to the first (same u)
            dp[2 * SP_K + j] += g;
        }
    }
    return xb;
}

__device__ __forceinline__ float sp_wrap(float z, float bound) {       // torch.remainder(z + b, 2 b) - b
    const float p = 2.f * bound;
    float r = fmodf(z + bound, p);
    if (r < 0.f) r += p;
    return r - bound;
}

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- the one-launch density kernels (spline_tile16.hip, spline_r8.h): the state tile stays in LDS ----------------------------
__device__ __forceinline__ void sp_identity_from_tile(const SplineDims& f, const float* __restrict__ Lp, const float* ZT,
                                                      float* A0, int AS, const Tid& t) {
    const float* meta = Lp + f.o_meta;
    const int n_id = (int)meta[M_CNT * 64];
    for (int e = t.tid; e < ROWS * AS; e += NTHREADS) {
        const int r = e / AS, i = e % AS;
        float v = 0.f;
        if (i < n_id) {
            v = ZT[r * 64 + (int)meta[M_IDF * 64 + i]];
            if (meta[M_PFON * 64 + i] != 0.f) {
                const int k = (int)meta[M_PFK * 64 + i];
                const float sc = meta[M_PFS * 64 + i];
                v = Lp[f.o_pfw + 2 * k] * sinf(sc * v) + Lp[f.o_pfw + 2 * k + 1] * cosf(sc * v);
            }
        }
        A0[e] = v;
    }
}

// parameters of coordinate j of chain row r in this layer: returns 0 (untouched), 1 (identity: unconditional), 2 (transformed)
__device__ __forceinline__ int sp_coord_params(const SplineDims& f, const float* __restrict__ Lp, const float* meta,
                                               const float* PT, int PS, int r, int j, float isq, float (&p)[SP_NP],
                                               int& pos) {
    const int pos_id = (int)meta[M_POSID * 64 + j], pos_tr = (int)meta[M_POSTR * 64 + j];
    if (pos_id >= 0) {
#pragma unroll
        for (int k = 0; k < SP_NP; ++k) p[k] = Lp[f.o_unc + pos_id * SP_NP + k];
        pos = pos_id;
        return 1;
    }
    if (pos_tr >= 0) {
#pragma unroll
        for (int k = 0; k < SP_NP; ++k) {
            const float v = PT[r * PS + pos_tr * SP_NP + k];
            p[k] = k < 2 * SP_K ? v * isq : v;
        }
        pos = pos_tr;
        return 2;
    }
    pos = -1;
    return 0;
}

}  // namespace fab
