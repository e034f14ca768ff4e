/* fabhip.h — C ABI of libfabhip.so: MI355X (gfx950) kernels for the fab-torch AIS / flow-density
 * hot path.  This is the drop-in boundary: plain device pointers + sizes, no torch types.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the field comment says "host";
 *   - all tensors are contiguous row-major float32 unless stated; indices are int64;
 *   - functions only ENQUEUE work on `stream` (a hipStream_t); they never allocate, never
 *     synchronise and never throw; scratch comes from the caller (`*_workspace_bytes`);
 *   - return value: FABHIP_OK or a negative FABHIP_E* code (see fabhip_strerror).
 *
 * Each entry point cites the reference (lollcat/fab-torch) interface it replaces.
 */
#ifndef FABHIP_H
#define FABHIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fabhip_stream_t; /* hipStream_t */

enum {
    FABHIP_OK = 0,
    FABHIP_EINVAL = -1,  /* bad shape / null pointer / misaligned buffer             */
    FABHIP_ENOTSUP = -2, /* dimension beyond compiled limits (dim<=64, width<=512)   */
    FABHIP_ELAUNCH = -3, /* hipGetLastError() != hipSuccess after a launch           */
    FABHIP_ENOSPC = -4   /* workspace too small                                      */
};

#define FABHIP_MAX_LAYERS 64
#define FABHIP_MAX_DIM 64
#define FABHIP_MAX_WIDTH 512

const char* fabhip_strerror(int code);
/* ABI revision of this header: bumped on every change of a struct layout or a function signature.  The host
 * binding compares it (and the struct sizes below) with what it was written against and refuses to run on a
 * mismatch, so that a stale library can never be driven with newer struct layouts. */
#define FABHIP_ABI_VERSION 227
int fabhip_version(void);
/* sizeof() of the argument structs as the library was compiled:
 * {fabhip_flow_params, fabhip_flow, fabhip_target, fabhip_point, fabhip_anneal, fabhip_hmc_args,
 *  fabhip_metropolis_args, fabhip_ais_args}. */
void fabhip_abi_sizes(int64_t out8[8]);

/* ------------------------------------------------------------------------------------------
 * RealNVP flow  (replaces normflows NormalizingFlow.sample / .log_prob as wrapped by
 * fab/wrappers/normflows.py:16-31, architecture of experiments/make_flow/make_normflow_model.py:11-30)
 * ---------------------------------------------------------------------------------------- */

/* Raw parameters in normflows / nn.Linear layout (weight[out][in]); host arrays of device pointers. */
typedef struct {
    int32_t dim, n_layers, width;
    const float* w1[FABHIP_MAX_LAYERS];     /* [width][d]          d = ceil(dim/2)            */
    const float* b1[FABHIP_MAX_LAYERS];     /* [width]                                        */
    const float* w2[FABHIP_MAX_LAYERS];     /* [width][width]                                 */
    const float* b2[FABHIP_MAX_LAYERS];     /* [width]                                        */
    const float* w3[FABHIP_MAX_LAYERS];     /* [2(dim-d)][width]   rows interleaved shift,scale */
    const float* b3[FABHIP_MAX_LAYERS];     /* [2(dim-d)]                                     */
    const float* lu_L[FABHIP_MAX_LAYERS];   /* [dim][dim] InvertibleAffine.L                  */
    const float* lu_U[FABHIP_MAX_LAYERS];   /* [dim][dim] InvertibleAffine.U                  */
    const float* log_S[FABHIP_MAX_LAYERS];  /* [dim]                                          */
    const float* sign_S[FABHIP_MAX_LAYERS]; /* [dim]                                          */
    const float* perm_P[FABHIP_MAX_LAYERS]; /* [dim][dim] permutation matrix                  */
    const float* loc;                       /* [dim] DiagGaussian.loc                         */
    const float* log_scale;                 /* [dim] DiagGaussian.log_scale                   */
    /* normflows ActNorm(dim) after layer k's InvertibleAffine (make_normflow_model.py:27-29, act_norm=True):
     * sampling direction z <- z * exp(s) + t, log_det += sum(s).  NULL (both) = no ActNorm after that layer. */
    const float* an_s[FABHIP_MAX_LAYERS];   /* [dim] ActNorm.s                                */
    const float* an_t[FABHIP_MAX_LAYERS];   /* [dim] ActNorm.t                                */
} fabhip_flow_params;

/* FAST MODE (off by default; NOT the parity path).  When on, the transition kernels (fabhip_hmc_transition,
 * fabhip_ais_run with HMC, fabhip_create_point and fabhip_flow_log_prob when they return gradients) run the two width x width GEMMs of every coupling
 * layer - 87 % of the flow's flops - on the bf16 matrix cores (v_mfma_f32_16x16x32_bf16, fp32 accumulation, weights
 * from a bf16 image every fabhip_flow_pack also writes, activations rounded to bf16 as they are fetched).  log q then
 * differs from the fp32 path at the 1e-3 .. 1e-2 level (the sampler stays a valid HMC-AIS sampler for that slightly
 * different density; fabhip_flow_sample, gradient-free density evaluations, the training path and Metropolis stay fp32).
 * fabhip_spline_log_prob with gradients does the same for the spline conditioner's hidden x hidden GEMMs.
 * Process-wide switch, returns the previous value.  SURVEY section 7's "fp32 parity mode and a fast mode". */
int fabhip_set_fast_mode(int on);
int fabhip_get_fast_mode(void);

/* Developer / test switches (A/B variants of one computation, diagnostics).  A plain table of ints inside the library:
 * initialised ONCE, when the library is loaded, from the environment variables named below, read by the launchers with
 * one load (nothing on a launch path calls getenv), changed at run time only through fabhip_set_option (returns the
 * previous value, or a negative FABHIP_E* code for an unknown key).  No reference counterpart (the reference has no
 * kernel variants); production code never sets them. */
#define FABHIP_OPT_TILE_SHAPE 0          /* FABHIP_TILE: chains per workgroup of the fused RealNVP transitions (4 = flow_r4.h,
                                            8 = flow_r8.h, 16 = flow_device.h tiles; a shape that does not exist for the flow
                                            falls back to 16) and of the 4x4x1 spline density kernel (8 / 16); 0 = by batch
                                            size (default) */
#define FABHIP_OPT_R4_STREAM 1           /* FABHIP_R4_STREAM: 4-chain tiles: 2 = fused stages on their own weight stream (flow_r4f.h: the
                                            D x D map multiplied together with the first / last conditioner Linear, coupling in the
                                            W3 epilogue; default where the image exists), 3 = the same with three items of every W x W
                                            stage prefetched into LDS during the short stages (opt-in: bit-identical to 2 and, measured,
                                            no faster - the copies' issue time lands on the short stages),
                                            1 = the round-3 stream (one stage per matrix), 0 = per-stage request groups.  The 8-chain tiles follow the same switch: >= 2 =
                                            their fused-stage stream (flow_r8.h, default), below = one stage per matrix */
#define FABHIP_OPT_SCAN_VARIANT 2        /* FABHIP_SCAN_VARIANT: fixed-point CDF scan, 3 = LDS-transposed (default), 0-2 = A/B */
#define FABHIP_OPT_SYSTEMATIC_VARIANT 3  /* FABHIP_SYSTEMATIC_VARIANT: 1 = fused systematic sampler (default), 0 = CDF in HBM */
#define FABHIP_OPT_SPLINE_STAGED 4       /* FABHIP_SPLINE_STAGED: 1 = per-layer spline kernels instead of the one-launch kernel */
#define FABHIP_OPT_TIMELINE 5            /* FABHIP_TIMELINE: 1 = workgroup 0 writes s_memtime stage stamps (fabhip_debug_timeline) */
#define FABHIP_OPT_SPLINE_MFMA 6         /* FABHIP_SPLINE_MFMA: spline density kernel for hidden widths padded to 256: 0 = the
                                            4x4x1 stream kernels (8 / 16 chains per workgroup by batch, or by TILE_SHAPE),
                                            16 = the 16x16x4 kernel */
#define FABHIP_OPT_SPLINE_LEAP 7         /* FABHIP_SPLINE_LEAP: fused spline transitions: 1 = one launch per leapfrog (half steps and
                                            the target inside the 4x4x1 spline density kernel, default), 0 = four launches */
#define FABHIP_OPT_FUSED_TAIL 8          /* FABHIP_FUSED_TAIL: AIS calls of <= 2048 chains: 1 = the compaction + ESS / log Z after the chain
                                            initialisation and after the last transition in ONE launch each (default), 0 = the six / five
                                            separate kernels (the same results, bit for bit) */
#define FABHIP_OPT_ADAPT_FOLD 9          /* FABHIP_ADAPT_FOLD: fused AIS calls on 4- / 8-chain tiles: 1 = the step-size rule runs in the LAST
                                            workgroup of every transition kernel (ticket; default), 0 = its own launch per transition.
                                            Spline family (round 5): 1 = an outer HMC step is L launches - begin inside the first
                                            leapfrog launch, accept + rule inside the last; 0 = L + 3 (the same results, bit for bit) */
#define FABHIP_OPT_PGRAD 10              /* FABHIP_PGRAD: parameter gradients from a RealNVP tape: 1 = the stream-K GEMM over all products of all
                                            layers (default; dense 64 x 64 / narrow tiles straight from HBM into the matrix cores, work cut
                                            into equal shares), 0 = the round-1 64 x 64 block kernel (A/B; other summation order) */
#define FABHIP_OPT_TAPE_TILES 11         /* FABHIP_TAPE_TILES: fabhip_flow_log_prob_tape: 0 = 8-chain stream tiles (flow_r8.h) where the flow has
                                            that image (default; inside fabhip_buffer_train_step with the minibatch arithmetic in the kernel's tail), 8 = the same
                                            tiles, the minibatch arithmetic as its own launch (A/B), 16 = always the 16-chain kernel (A/B; other summation order) */
#define FABHIP_OPT_COUNT 12
int fabhip_set_option(int key, int value);
int fabhip_get_option(int key);

/* Number of floats of the MFMA-tiled parameter image for a (dim, n_layers, width) flow. */
int64_t fabhip_flow_packed_floats(int32_t dim, int32_t n_layers, int32_t width);

/* Assemble W = P L U and W^-1 (fp64 triangular inverses) per layer and re-tile every matrix
 * (and its transpose) into v_mfma_f32_16x16x4_f32 B-operand order.  Call after each optimiser step. */
int fabhip_flow_pack(const fabhip_flow_params* params, float* packed, fabhip_stream_t stream);
/* Same without the W^-1 matrices (their float64 triangular inverses are 80 % of the packing time): enough for
 * fabhip_flow_log_prob / _log_prob_tape / the transition kernels between two optimiser steps of a minibatch loop;
 * fabhip_flow_sample and fabhip_ais_run need a full fabhip_flow_pack first. */
int fabhip_flow_pack_density(const fabhip_flow_params* params, float* packed, fabhip_stream_t stream);
/* The image for the TRAINING forward only (round 6): what fabhip_flow_log_prob_tape reads - the assembled affine maps, the 16-chain
 * tiles with the biases and, where the flow has them, the 8-chain stream tiles; ~1/4 of the launches of a density pack.  Used between
 * the optimiser steps of the replay-buffer minibatches (fabhip_buffer_train_step); any other consumer needs fabhip_flow_pack /
 * fabhip_flow_pack_density afterwards. */
int fabhip_flow_pack_train(const fabhip_flow_params* params, float* packed, fabhip_stream_t stream);

/* `precision`: per CALL choice between the fp32 parity kernels and fast mode (below) for the entry points that have both -
 * FABHIP_PRECISION_DEFAULT (0, what a zero-initialised struct gets) follows the process default of fabhip_set_fast_mode,
 * _FP32 / _FAST override it, so two samplers of one process can differ. */
enum { FABHIP_PRECISION_DEFAULT = 0, FABHIP_PRECISION_FP32 = 1, FABHIP_PRECISION_FAST = 2 };
typedef struct {
    int32_t dim, n_layers, width;
    int32_t precision;   /* FABHIP_PRECISION_* */
    const float* packed; /* fabhip_flow_pack output */
} fabhip_flow;

/* x, log_q = flow.sample_and_log_prob given base noise eps[B][dim] ~ N(0,1)
 * (fab/wrappers/normflows.py:16-18 -> NormalizingFlow.sample). */
int fabhip_flow_sample(const fabhip_flow* flow, const float* eps, float* x, float* log_q, int64_t B,
                       fabhip_stream_t stream);

/* log_q[B] = flow.log_prob(x[B][dim]); if grad_x != NULL also d log_q / d x [B][dim]
 * (fab/wrappers/normflows.py:23-24 and the autograd call of fab/sampling_methods/base.py:50-56). */
int fabhip_flow_log_prob(const fabhip_flow* flow, const float* x, float* log_q, float* grad_x, int64_t B,
                         fabhip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Circular / linear-tail rational-quadratic spline COUPLING flow (the alanine-dipeptide flow of
 * experiments/make_flow/make_aldp_model.py:57-71,121-134,146-167: n_layers x normflows
 * CircularCoupledRationalQuadraticSpline(dim, 1 block, hidden, ind_circ, tail_bound, 8 bins, mask) with PeriodicShift /
 * PeriodicWrap layers and a UniformGaussian base; replaces NormalizingFlow.log_prob / .sample behind
 * fab/wrappers/normflows.py:16-31).  dim <= 64, hidden <= 256, 8 bins, one residual block per conditioner.
 *
 * Per layer, raw parameters in normflows / nn.Linear layout (weight[out][in]):
 *   w0 [hidden][n_id], b0 [hidden]            transform_net.initial_layer
 *   wa, wb [hidden][hidden], ba, bb [hidden]  transform_net.blocks.0.linear_layers.{0,1}
 *   wf [25 n_tr][hidden], bf [25 n_tr]        transform_net.final_layer (per transformed coordinate: 8 widths, 8 heights,
 *                                             9 knot derivatives)
 *   pfw [n_pf][2] (may be NULL)               transform_net.preprocessing.weights (periodic features)
 *   uw, uh [n_id][8], ud [n_id][9]            unconditional_transform.unnormalized_{widths,heights,derivatives}
 *   meta [12][64] floats: row 0 identity coordinate indices (n_id valid), 1 transformed coordinate indices (n_tr valid),
 *     2 circular flag per coordinate, 3 tail bound per coordinate, 4 periodic-feature flag per identity position,
 *     5 its scale pi / bound, 6 its row in pfw, 7/8 shift and on-flag applied BEFORE this layer in the log_prob direction
 *     (z <- wrap(z - shift): PeriodicShift.inverse / PeriodicWrap.inverse), 9/10 shift and on-flag applied AFTER this layer
 *     in the sampling direction (PeriodicShift.forward), 11: {n_id, n_tr, n_pf}.
 * base_scale [dim], base_circ [dim] (0/1): UniformGaussian (uniform on [-scale/2, scale/2] for circular coordinates).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t dim, n_layers, hidden;
    const float* meta[FABHIP_MAX_LAYERS];
    const float* w0[FABHIP_MAX_LAYERS];
    const float* b0[FABHIP_MAX_LAYERS];
    const float* wa[FABHIP_MAX_LAYERS];
    const float* ba[FABHIP_MAX_LAYERS];
    const float* wb[FABHIP_MAX_LAYERS];
    const float* bb[FABHIP_MAX_LAYERS];
    const float* wf[FABHIP_MAX_LAYERS];
    const float* bf[FABHIP_MAX_LAYERS];
    const float* pfw[FABHIP_MAX_LAYERS];
    const float* uw[FABHIP_MAX_LAYERS];
    const float* uh[FABHIP_MAX_LAYERS];
    const float* ud[FABHIP_MAX_LAYERS];
    const float* base_scale;
    const float* base_circ;
} fabhip_spline_params;

typedef struct {
    int32_t dim, n_layers, hidden;
    int32_t precision;   /* FABHIP_PRECISION_* (the density + gradient kernel has a fast variant) */
    const float* packed; /* fabhip_spline_pack output */
} fabhip_spline_flow;

int64_t fabhip_spline_packed_floats(int32_t dim, int32_t n_layers, int32_t hidden);
/* development aid (FABHIP_TIMELINE=1): s_memtime stamps of one layer of the one-launch density kernel */
int fabhip_debug_spline_timeline(int64_t* host_out, int32_t n);
int fabhip_spline_pack(const fabhip_spline_params* params, float* packed, fabhip_stream_t stream);
size_t fabhip_spline_workspace_bytes(int32_t dim, int32_t n_layers, int32_t hidden, int64_t B, int32_t with_grad);
/* log_q[B] = flow.log_prob(x[B][dim]) and, if grad_x != NULL, d log_q / dx [B][dim] (reverse sweep through all layers). */
int fabhip_spline_log_prob(const fabhip_spline_flow* flow, const float* x, float* log_q, float* grad_x, int64_t B,
                           void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
/* Training tape of the spline flow (the backward of `flow.log_prob(x)` w.r.t. the flow parameters in the forward-KL
 * term of the FAB loss, fab/core.py:114-127, for the normflows spline family).  One call computes log_q, d log_q / dx
 * (required) and writes, per coupling layer l at tape + l * out16[1], row-major [B][width] matrices at offsets
 *   out16[2] XI  [B][64]   raw identity coordinates         out16[3] A0  [B][64]  after the periodic features
 *   out16[4] dA0 [B][64]   cotangent of A0                  out16[5] R0  [B][Wp]  relu(h0)
 *   out16[6] R1  [B][Wp]   relu(t)                          out16[7] H1  [B][Wp]  h1 (input of the final layer)
 *   out16[8] dH1 out16[9] dT out16[10] dH0 [B][Wp]          cotangents of h1, t (ReLU-masked), h0
 *   out16[11] dP [B][NFP]  cotangent of the conditioner output (columns >= 25 n_transform are 0)
 *   out16[12] dU [B][out16[15]] cotangent of the unconditional parameters, [identity position][25]
 * with out16[0] = total floats, out16[13] = Wp, out16[14] = NFP.  All cotangents are for seed 1 per sample: the
 * gradient of sum_b c_b log q(x_b) w.r.t. a Linear's weight is (c * cotangent)^T @ activation - plain GEMMs over the
 * tape, left to the caller's BLAS (rocBLAS; fab_torch_amd/spline_flow.py uses torch.mm). */
int fabhip_spline_tape_layout(int32_t dim, int32_t n_layers, int32_t hidden, int64_t B, int64_t out16[16]);
/* The GEMMs over a tape: for L layers of one shape  C[l][p][q] = sum_b coef[b] Y[l][b][p] X[l][b][q]  (Y: cotangents
 * [B][ldy], X: activations [B][ldx], layer l at Y + l * y_layer_stride / X + l * x_layer_stride; C row-major [L][P][Q])
 * and, if colsum != NULL, the bias gradients colsum[l][p] = sum_b coef[b] Y[l][b][p] - the backward of a Linear
 * (loss.backward() through flow.log_prob, fab/train_with_prioritised_buffer.py:162-177) on the fp32 matrix cores,
 * deterministic summation order.  ldy / ldx multiples of 4 and 16-byte aligned bases take the vector path. */
int fabhip_tape_gemm(const float* Y, int64_t y_layer_stride, int32_t ldy, int32_t P, const float* X, int64_t x_layer_stride,
                     int32_t ldx, int32_t Q, const float* coef, int64_t B, int32_t L, float* C, float* colsum,
                     fabhip_stream_t stream);
int fabhip_spline_log_prob_tape(const fabhip_spline_flow* flow, const float* x, float* log_q, float* grad_x, int64_t B,
                                float* tape, int64_t tape_floats, void* workspace, size_t workspace_bytes,
                                fabhip_stream_t stream);
/* The backward of `x, log_q = flow.sample_and_log_prob()` w.r.t. the parameters and the base noise (the reparameterised baseline
 * losses, fab/core.py:130-152 with the spline flow of experiments/make_flow/make_aldp_model.py), by the implicit function theorem
 * on the log_prob direction S (x = S^-1(z0; theta), z0 = the base sample): for cotangents gx of x and gl of log_q (either nullable),
 *   d/d theta = gl * d log q(x) / d theta |_x  -  v_l^T dS_l / d theta_l,   v = (dS/dx)^-T (gx + gl * d log q / dx).
 * The call re-runs the sampler from (u, eps) keeping every layer's state (the sweeps linearise where the sample was made, not on a
 * trajectory re-derived from the rounded x), runs the log_prob direction's reverse sweep on them (tape_density: seed 1 per sample,
 * as fabhip_spline_log_prob_tape writes it) and carries v from the x side to the base side (tape_inverse, same layout).  The
 * parameter gradients are the tape GEMMs of tape_density with coefficients gl plus those of tape_inverse with coefficients 1.
 * v_x [B][dim]: scratch, on return v at x.  v_base (nullable) [B][dim]: v at the base side = the cotangent of z0.
 * Workspace: fabhip_spline_workspace_bytes(.., with_grad = 1); each tape fabhip_spline_tape_layout's out16[0] floats. */
int fabhip_spline_sample_vjp_tape(const fabhip_spline_flow* flow, const float* u, const float* eps, const float* gx, const float* gl,
                                  float* v_x, float* v_base, int64_t B, float* tape_density, float* tape_inverse,
                                  int64_t tape_floats, void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
/* x, log_q = flow.sample given u[B][dim] ~ U(0,1) (circular coordinates) and eps[B][dim] ~ N(0,1) (the others). */
int fabhip_spline_sample(const fabhip_spline_flow* flow, const float* u, const float* eps, float* x, float* log_q,
                         int64_t B, void* workspace, size_t workspace_bytes, fabhip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Flow training path — the backward of `flow.log_prob(x)` w.r.t. the parameters, i.e. what
 * `loss.backward()` does in fab/train_with_prioritised_buffer.py:162-177 (loss = -mean(w_adjust * log_q_x))
 * and for fab/core.py:112-118 (fab_alpha_div_inner).  Two calls:
 *   fabhip_flow_log_prob_tape : log_q (and optionally d log_q / dx) exactly as fabhip_flow_log_prob, plus a
 *                               tape of per-layer activations / deltas in caller-owned device memory;
 *   fabhip_flow_param_grad    : grads[theta] = sum_b coef[b] * d log_q(x_b) / d theta for every parameter,
 *                               coef = d loss / d log_q (autograd's grad_output), written into one flat image:
 *                               per layer [w1 | b1 | w2 | b2 | w3 | b3 | L | U | log_S] (each in the shape of
 *                               the fabhip_flow_params tensor of that name), then loc, log_scale; when
 *                               params->an_s is set (ActNorm flows) then per layer [an_s | an_t] - `grads` must
 *                               then hold out15[14] floats instead of out15[12].
 * fabhip_flow_grad_layout fills {layer_stride, w1, b1, w2, b2, w3, b3, L, U, log_S (offsets inside a layer
 * block), loc, log_scale (absolute offsets), total, an_base (absolute offset of layer 0's [an_s | an_t] pair, the
 * pairs are 2 dim floats apart), total with ActNorm}, all in floats.
 * ---------------------------------------------------------------------------------------- */
int64_t fabhip_flow_grad_floats(int32_t dim, int32_t n_layers, int32_t width);
int fabhip_flow_grad_layout(int32_t dim, int32_t n_layers, int32_t width, int64_t* out15);
size_t fabhip_flow_tape_bytes(int32_t dim, int32_t n_layers, int32_t width, int64_t B);
/* Layout of the tape (floats): row-major [Bp x width] matrices per layer block, then the base block TB.
 * out18 = {Bp, wz, w1, wh, wp, we, wb (row widths of ZA/GZ, Z1, H1/H2, DP, E1/E2, TB),
 *          o_ZA, o_GZ, o_Z1, o_H1, o_H2, o_DP, o_E2, o_E1 (offsets inside a layer block), layer_stride, o_TB, total}.
 * H1 / H2 hold the hidden activations AFTER the ReLU (their first `width` columns), i.e. the ReLU decisions the
 * gradients were computed with. */
int fabhip_flow_tape_layout(int32_t dim, int32_t n_layers, int32_t width, int64_t B, int64_t* out18);
int fabhip_flow_log_prob_tape(const fabhip_flow* flow, const float* x, float* log_q, float* grad_x, int64_t B,
                              void* tape, size_t tape_bytes, fabhip_stream_t stream);
/* The same with the batch read in place from a larger matrix: batch row g is row rows[g] of x (`self.buffer.x[indices]` of
 * fab/utils/prioritised_replay_buffer.py:98 without materialising the gather). */
int fabhip_flow_log_prob_tape_rows(const fabhip_flow* flow, const float* x, const int64_t* rows, float* log_q, float* grad_x,
                                   int64_t B, void* tape, size_t tape_bytes, fabhip_stream_t stream);
int fabhip_flow_param_grad(const fabhip_flow_params* params, const fabhip_flow* flow, const void* tape,
                           size_t tape_bytes, const float* coef, int64_t B, float* grads, fabhip_stream_t stream);
/* Backward of the SAMPLING direction - `loss.backward()` through `flow.sample_and_log_prob` for the reparameterised
 * baseline losses flow_reverse_kl / flow_alpha_2_div_nis (fab/core.py:130-152).  Given x = the samples fabhip_flow_sample
 * returned, grad_x = d loss / dx [B][dim] and grad_log_q = d loss / d log_q [B], one sweep x -> eps writes the same tape
 * as fabhip_flow_log_prob_tape (same size and layout) with the sampling direction's cotangents, such that
 * fabhip_flow_param_grad(params, flow, tape, coef = ones[B], B, grads) returns d loss / d theta.  grad_eps (nullable)
 * receives d loss / d eps.  `flow->packed` must come from fabhip_flow_pack (with the inverses). */
int fabhip_flow_sample_grad_tape(const fabhip_flow* flow, const float* x, const float* grad_x, const float* grad_log_q,
                                 float* grad_eps, int64_t B, void* tape, size_t tape_bytes, fabhip_stream_t stream);

/* One optimiser step on a flat parameter image (the layout of fabhip_flow_grad_layout): global-norm clipping
 * (torch.nn.utils.clip_grad_norm_(params, max_norm), fab/train_with_prioritised_buffer.py:174; max_norm <= 0 = off)
 * followed by Adam (torch.optim.Adam defaults: no weight decay, no amsgrad).  The total gradient norm is written
 * to grad_norm_out (device, may be NULL); when it is not finite nothing is updated — the reference's "nan grad
 * norm" skip (:175-179) without a host round trip.  m, v: Adam moments, same length.  step_count: device int32,
 * the number of applied steps so far (drives the bias correction); incremented here when the update is applied. */
size_t fabhip_adam_workspace_bytes(int64_t n);
int fabhip_adam_clip_step(float* theta, const float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                          float beta2, float eps, int32_t* step_count, float max_norm, float* grad_norm_out,
                          void* workspace, size_t workspace_bytes, fabhip_stream_t stream);

/* ONE gradient step on ONE minibatch of the prioritised replay buffer - the body of the minibatch loop of
 * fab/train_with_prioritised_buffer.py:158-185 with the buffer's `adjust` (fab/utils/prioritised_replay_buffer.py:117-131),
 * enqueued without a host synchronisation:
 *   (repack != 0) the training image of the current parameters (fabhip_flow_pack_train);
 *   log_q = flow.log_prob(x) with the tape - x either [B][dim] (rows == NULL) or the buffer's x with the minibatch's row indices;
 *   log_w_adjust = (1 - alpha) (log_q - log_q_old), w = clip(exp(log_w_adjust), max = w_adjust_max_clip) (<= 0: no clip),
 *   loss = -mean(w log_q), coef = -w / B (w is detached in the reference's loss; NaN-poisoned when the loss is not finite, which the
 *   optimiser's finite-norm test turns into the reference's skipped update, :172-181);
 *   (buf_log_w != NULL) buffer.adjust on the minibatch's rows: log_w += log_w_adjust and log_q_old = log_q where both are finite,
 *   log_w = -inf elsewhere (the reference adjusts after the optimiser step with the same values, :184-185; needs unique rows:
 *   sampling without replacement);
 *   grads = sum_b coef_b d log q(x_b) / d theta (fabhip_flow_param_grad), then fabhip_adam_clip_step on (theta, m, v).
 * `params` point INTO theta (the flat layout of fabhip_flow_grad_layout: FlatAdam).  log_q_old: [B] (log_q_old_rows = 0) or the
 * buffer's log_q_old, read at rows[b] (= 1).  stats[8] (device): loss, mean / min / max of exp(log_w_adjust) before the clip,
 * mean(log_q), gradient norm - the reference's logging keys (:188-196); the norm is NaN for a minibatch skipped for its non-finite
 * loss (the reference computes none there, :172-173: the caller keeps the last one it saw, as PrioritisedBufferTrainer does).
 * stats[5] alone therefore does not tell "loss skipped" from "finite loss whose gradient norm is NaN" (:175-179, also no update):
 * a caller that needs the difference tests stats[0] for finiteness first.  struct_bytes = sizeof(fabhip_train_step_args). */
typedef struct {
    size_t struct_bytes;
    const fabhip_flow_params* params;
    float* packed;
    int32_t repack, log_q_old_rows;
    const float* x;
    const int64_t* rows;
    const float* log_q_old;
    int64_t B;
    float alpha, w_adjust_max_clip;
    float *buf_log_w, *buf_log_q_old;
    float *log_q, *log_w_adjust, *coef, *grads, *stats;      /* outputs: [B], [B], [B], [n_params], [8] */
    float *theta, *m, *v;
    int64_t n_params;
    float lr, beta1, beta2, eps, max_grad_norm;
    int32_t* step_count;
    void* workspace;                                         /* 256-byte aligned */
    size_t workspace_bytes;
} fabhip_train_step_args;
/* PrioritisedReplayBuffer.add (fab/utils/prioritised_replay_buffer.py:71-85) in one launch: the n new rows go to rows
 * (start + i) mod max_length of the ring (x [max_length][dim], log_w, log_q_old [max_length]). */
int fabhip_buffer_add(const float* x, const float* log_w, const float* log_q_old, int64_t n, int32_t dim, int64_t start,
                      int64_t max_length, float* buf_x, float* buf_log_w, float* buf_log_q_old, fabhip_stream_t stream);
/* PrioritisedReplayBuffer.sample's row selection without replacement (:10-17, :88-97) given the uniform draws: the k rows with
 * the largest log_w + Gumbel(u_gumbel[n]) (fabhip_topk), in a pseudo-random order (`indices[torch.randperm(k)]`): a keyed
 * bijection of [0, k) - four Feistel rounds with cycle walking - whose round keys come from the four uniforms u_order[4]. */
size_t fabhip_buffer_sample_workspace_bytes(int64_t n, int64_t k);
int fabhip_buffer_sample(const float* log_w, const float* u_gumbel, const float* u_order, int64_t n, int64_t k, int64_t* idx_out,
                         void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
size_t fabhip_train_step_workspace_bytes(int32_t dim, int32_t n_layers, int32_t width, int64_t B, int64_t n_params);
int fabhip_buffer_train_step(const fabhip_train_step_args* args, fabhip_stream_t stream);
/* What fabhip_buffer_train_step runs for this flow under the current FABHIP_OPT_TAPE_TILES (host-only, read-only; the dispatcher
 * takes its decision from the same function): out3 = {rows per workgroup of the tape kernel (8 or 16), hidden column groups
 * G = padded width / 64, 1 if the minibatch arithmetic runs in the tape kernel's tail / 0 if k_buffer_minibatch is launched}. */
int fabhip_train_step_plan(int32_t dim, int32_t n_layers, int32_t width, int64_t* out3);

/* ------------------------------------------------------------------------------------------
 * Targets (fab/target_distributions/many_well.py:81-90, double_well.py:44-58, gmm.py:57-66)
 * ---------------------------------------------------------------------------------------- */
/* FABHIP_TARGET_QUARTIC (ABI 224): coupled quartic sites (lattice phi^4, coupled double wells, correlated Gaussians),
 *   log p(x) = - sum_j (a_j x_j + b_j x_j^2 + c_j x_j^4) - 1/2 sum_j x_j (J x)_j - log_norm,   1 <= dim <= FABHIP_MAX_DIM,
 * with J SYMMETRIC (the kernels read J[k][j] for (J x)_j and do not check it).  NaN / inf coordinates propagate. */
/* FABHIP_TARGET_ROTOR (ABI 227): coupled rotors (lattice XY, torsion angles with Fourier terms, harmonic line sites),
 *   t_j = x_j r_j,  w_j = t_j - rint(t_j),  theta_j = 2 pi w_j,  d_jn = (w_j - w_k) - rint(w_j - w_k) with k = k_jn,
 *   log p(x) = sum_j [sum_{m=1..3} (A_mj cos m theta_j + B_mj sin m theta_j) - l_j x_j - q_j x_j^2]
 *              + 1/2 sum_j sum_{n<NB} kap_jn cos(2 pi d_jn) - log_norm,                         1 <= dim <= FABHIP_MAX_DIM.
 * r_j = 1 / period of a periodic site, 0 of a site on the line.  The neighbour table is the row form of a SYMMETRIC coupling
 * with a zero diagonal: every bond listed from both ends (the gradient relies on it and the kernels do not check it), unused
 * slots padded with k = j, kap = 0.  Every index entry must be a FINITE float (the kernels convert it to an integer; a NaN or inf
 * entry has no defined conversion); a finite index outside 0 .. dim - 1 is clamped.  NaN / inf coordinates propagate. */
enum { FABHIP_TARGET_MANYWELL = 1, FABHIP_TARGET_GMM = 2, FABHIP_TARGET_QUARTIC = 3, FABHIP_TARGET_ROTOR = 4 };

typedef struct {
    int32_t kind, dim;
    float a, b, c;       /* many well: energy a x + b x^2 + c x^4 on even dims, x^2/2 on odd     */
    float log_norm;      /* subtracted from log p (0 unless `normalised`); many well, quartic and rotor */
    int32_t n_mix;       /* GMM: number of equally weighted components; rotor: the neighbour table's     */
                         /* width NB, 1 .. 63; unused otherwise                                          */
    const float* locs;   /* GMM: [n_mix][dim]; quartic: the coupling J, [dim][dim], symmetric; rotor:    */
                         /* [2 NB][dim], rows 0 .. NB - 1 the neighbour indices as floats, rows NB ..    */
                         /* 2 NB - 1 the couplings                                                       */
    const float* scales; /* GMM: [n_mix][dim] diagonal of scale_tril; quartic: the site coefficients     */
                         /* [3][dim], rows a, b, c; rotor: [9][dim], rows A1 A2 A3 B1 B2 B3 r l q        */
} fabhip_target;

int fabhip_target_log_prob(const fabhip_target* target, const float* x, float* log_p, float* grad_x,
                           int64_t B, fabhip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Point (fab/sampling_methods/base.py:7-47) as a struct of device arrays.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    float* x;          /* [B][dim] */
    float* log_q;      /* [B]      */
    float* log_p;      /* [B]      */
    float* grad_log_q; /* [B][dim] or NULL (Metropolis) */
    float* grad_log_p; /* [B][dim] or NULL              */
} fabhip_point;

/* create_point(x, ...) with gradients: fab/sampling_methods/base.py:59-72. point.x is read. */
int fabhip_create_point(const fabhip_flow* flow, const fabhip_target* target, const fabhip_point* point,
                        int32_t with_grad, int64_t B, fabhip_stream_t stream);

/* Coefficients of the annealed density (fab/sampling_methods/base.py:76-118), float32:
 *   log pi_beta = c_q log_q + c_p log_p ;  grad = g_q grad_log_q + g_p grad_log_p
 * (g_p = 2 beta when not p_target: the reference's hard-coded factor, base.py:116). */
/* C callers: ZERO-INITIALISE fabhip_flow / fabhip_spline_flow (`fabhip_flow f = {0};`) before filling them in.  `precision`
 * (ABI 207) sits where padding used to be, so sizeof did not change and fabhip_abi_sizes cannot tell a caller compiled against
 * the older header apart - only FABHIP_ABI_VERSION can; an uninitialised value of 1 / 2 would silently select a precision. */
typedef struct {
    float c_q, c_p, g_q, g_p;
} fabhip_anneal;
void fabhip_anneal_coefs(double beta, double alpha, int32_t p_target, fabhip_anneal* out);

/* ------------------------------------------------------------------------------------------
 * HMC transition  (fab/sampling_methods/transition_operators/hmc.py:105-202)
 * One call = HamiltonianMonteCarlo.transition(point, i, beta): n_outer x (L leapfrogs,
 * Metropolis accept, in-place commit, step-size adaptation) and, if `log_w`, the AIS
 * log-weight increment of ais.py:93-100 with the coefficients `next`.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    fabhip_flow flow;
    fabhip_target target;
    fabhip_point point;     /* in/out, mutated in place like the reference           */
    int64_t B;              /* rows allocated                                        */
    const int32_t* n_valid; /* device scalar: rows in use (NULL -> B)                */
    fabhip_anneal cur;      /* beta_j                                                */
    fabhip_anneal next;     /* beta_{j+1} (used when log_w != NULL)                  */
    float* log_w;           /* [B] in/out or NULL                                    */
    const float* noise_p;   /* [n_outer][B][dim] ~ N(0,1)   (hmc.py:134)             */
    const float* noise_e;   /* [n_outer][B]      ~ Exp(1)   (hmc.py:118)             */
    float* epsilons;        /* -> epsilons[i-1][0..n_outer)  (state buffer, updated) */
    float* common_epsilon;  /* [1] state buffer, updated                             */
    const float* mass;      /* [dim]                                                 */
    int32_t n_outer, L;
    float max_grad, target_p_accept;
    int32_t tune;           /* 1 = adapt step sizes (not eval_mode)                  */
    float* p_accept;        /* [n_outer] out (mean acceptance prob) or NULL          */
    float* avg_distance;    /* [1] out, store_info's distance statistic, or NULL     */
    void* workspace;
    size_t workspace_bytes;
    /* Sharded chains: NULL = adapt from this call's own chains (above).  Otherwise the step sizes, p_accept
     * and avg_distance are left alone and the call publishes its acceptance statistics as ONE slab of
     * fabhip_hmc_partials_floats(B) floats - per 16-chain block the sum of min(1, acceptance) and of store_info's
     * distance, then the number of chains in use: [acc[nblk] | dist[nblk] | n] - which the caller all-gathers over the
     * ranks and hands to fabhip_hmc_adapt_gathered.  Requires n_outer == 1 (every shipped config, setup_run.py:190). */
    float* partials;
} fabhip_hmc_args;

size_t fabhip_hmc_workspace_bytes(int64_t B, int32_t dim, int32_t n_outer);
int fabhip_hmc_transition(const fabhip_hmc_args* args, fabhip_stream_t stream);

/* Step-size adaptation of hmc.py:122-123,162-170 on the mean acceptance of ALL chains of a sharded batch: `gathered` =
 * the partials slabs of n_ranks ranks in rank order (each fabhip_hmc_partials_floats(B_rank) floats, equal B_rank).
 * The sums run over ranks, then blocks, in order - with shards that are multiples of 16 chains exactly the sequence a
 * single device adds for the whole batch, so every rank ends up with the single-device step sizes bit for bit. */
int64_t fabhip_hmc_partials_floats(int64_t B);
int fabhip_hmc_adapt_gathered(const float* gathered, int32_t n_ranks, int64_t B_rank, float* epsilon, float* common_epsilon,
                              float target_p_accept, int32_t tune, float* p_accept, float* avg_distance,
                              fabhip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Metropolis transition (fab/sampling_methods/transition_operators/metropolis.py:51-74)
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    fabhip_flow flow;
    fabhip_target target;
    fabhip_point point;      /* grads unused */
    int64_t B;
    const int32_t* n_valid;
    fabhip_anneal cur, next;
    float* log_w;
    const float* noise_x;    /* [n_updates][B][dim] ~ N(0,1)  (metropolis.py:57) */
    const float* noise_u;    /* [n_updates][B]      ~ U(0,1)  (metropolis.py:65) */
    float* noise_scalings;   /* -> noise_scalings[i-1][0..n_updates), updated    */
    int32_t n_updates;       /* >= 1, no upper bound (as the reference); every update's scaling is adapted */
    float target_p_accept;
    int32_t tune;            /* adjust_step_size and not eval_mode               */
    void* workspace;
    size_t workspace_bytes;
} fabhip_metropolis_args;

/* Noise-scaling adaptation of metropolis.py:68-73 on the mean acceptance of ALL chains of a sharded batch.  The scaling
 * of (transition i, update n) is read by that update only and adjusted right after it: nothing later in the same AIS call
 * reads the adjusted value, so a sharded call defers the rule of all M transitions to ONE gather at its end.  `gathered` =
 * the slabs of n_ranks ranks in rank order, each fabhip_metropolis_partials_floats(B_rank, M, n_updates) floats:
 * per transition [n_updates][ceil(B_rank / 16)] sums of min(1, acceptance) per 16-chain block, then the chains in use
 * (fabhip_ais_phase with `partials`).  Sums run over ranks, then blocks, in order: with shards that are multiples of 16
 * chains exactly what one device adds, so every rank ends with the single-device noise_scalings [M][n_updates] bit for bit. */
int64_t fabhip_metropolis_partials_floats(int64_t B, int32_t M, int32_t n_updates);
int fabhip_metropolis_adapt_gathered(const float* gathered, int32_t n_ranks, int64_t B_rank, int32_t M, int32_t n_updates,
                                     float* noise_scalings, float target_p_accept, int32_t tune, fabhip_stream_t stream);

size_t fabhip_metropolis_workspace_bytes(int64_t B, int32_t dim, int32_t n_updates);
int fabhip_metropolis_transition(const fabhip_metropolis_args* args, fabhip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Generic plug-in path: transitions for ANY `Distribution` / `LogProbFunc` plug-in (fab/types_.py:5-27,
 * fab/sampling_methods/ais.py:22-30).  The caller evaluates log q, log p and their gradients with the plug-ins' own
 * code (create_point, fab/sampling_methods/base.py:50-72); everything else of a transition runs here as
 * elementwise kernels.  One workspace of fabhip_generic_workspace_bytes(B, dim) carries the trajectory state
 * (x, p, grad U, -U-K of the current point, acceptance partials) between the calls of one outer step:
 *
 *   HMC outer step n (hmc.py:129-160):
 *     fabhip_hmc_generic_begin(start, cur, ...)        p0 = noise_p * mass, grad U(start), x <- start.x
 *     L x { fabhip_hmc_generic_leap_pre(... x_out)     p -= eps gradU/2 ; x += eps/mass p ; x_out <- x
 *           [caller: log q, log p, gradients at x_out]
 *           fabhip_hmc_generic_leap_post(gq, gp, ...)  gradU <- clamp(-(g_q gq + g_p gp)) ; p -= eps gradU/2 }
 *     fabhip_hmc_generic_accept(prop, cur, ...)        Metropolis test with noise_e, in-place commit into `cur`,
 *                                                      log_w increment (if log_w), step-size adaptation, logging
 *   (`start` = `cur` for n = 0; for n > 0 the reference continues from the previous PROPOSAL, hmc.py:133-142.)
 *
 *   Metropolis update n (metropolis.py:51-74): fabhip_metropolis_generic_propose -> [caller: log q, log p at x_new]
 *     -> fabhip_metropolis_generic_accept (prev_log_prob = fabhip_anneal_log_prob of the point BEFORE the first
 *     update, never refreshed: the reference's stale x_prev_log_prob).
 * ---------------------------------------------------------------------------------------- */
size_t fabhip_generic_workspace_bytes(int64_t B, int32_t dim);
int fabhip_hmc_generic_begin(const fabhip_point* start, const fabhip_point* cur, int64_t B, int32_t dim,
                             fabhip_anneal c, const float* noise_p, const float* mass, float max_grad,
                             void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
int fabhip_hmc_generic_leap_pre(int64_t B, int32_t dim, const float* eps_ptr, const float* ceps_ptr, const float* mass,
                                float* x_out, void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
int fabhip_hmc_generic_leap_post(int64_t B, int32_t dim, const float* grad_log_q, const float* grad_log_p,
                                 fabhip_anneal c, float max_grad, const float* eps_ptr, const float* ceps_ptr,
                                 void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
int fabhip_hmc_generic_accept(const fabhip_point* prop, const fabhip_point* cur, int64_t B, int32_t dim, fabhip_anneal c,
                              fabhip_anneal next, float* log_w, const float* noise_e, const float* mass,
                              float* eps_ptr, float* ceps_ptr, float target_p_accept, int32_t tune, float* p_accept,
                              float* avg_distance, void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
/* out[i] = c_q log_q[i] + c_p log_p[i]  (get_intermediate_log_prob, base.py:76-97) */
int fabhip_anneal_log_prob(const float* log_q, const float* log_p, int64_t n, fabhip_anneal c, float* out,
                           fabhip_stream_t stream);
/* log_w += pi_next(point) - pi_c(point)  (ais.py:93-100) */
int fabhip_log_w_update(const float* log_q, const float* log_p, int64_t n, fabhip_anneal c, fabhip_anneal next,
                        float* log_w, fabhip_stream_t stream);
/* The first weight of a chain whose FABHIP_AIS_INIT ran with betas[1] = 0 (adaptive schedules, fabhip_next_beta): there
 * log_w = log_q - log_q0 exactly (two float32 values of one density, Sterbenz), so this writes
 *     log_w = pi_next(point) - (log_q - log_w)  =  pi_next(point) - log_q0
 * - the bits FABHIP_AIS_INIT writes when it is given betas[1] = beta_1 itself. */
int fabhip_log_w_first(const float* log_q, const float* log_p, int64_t n, fabhip_anneal next, float* log_w,
                       fabhip_stream_t stream);
int fabhip_metropolis_generic_propose(const float* x, const float* noise_x, const float* scale_ptr, int64_t B, int32_t dim,
                                      float* x_new, fabhip_stream_t stream);
int fabhip_metropolis_generic_accept(const float* x_new, const float* new_log_q, const float* new_log_p,
                                     const fabhip_point* cur, const float* prev_log_prob, const float* noise_u,
                                     int64_t B, int32_t dim, fabhip_anneal c, float* scale_ptr, float target_p_accept,
                                     int32_t tune, void* workspace, size_t workspace_bytes, fabhip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Whole AIS call  (fab/sampling_methods/ais.py:53-105): sample the flow, create the point,
 * initial log-weights, NaN/inf filtering (stable compaction, ais.py:190-213), M transitions
 * with log-weight accumulation, final filtering, ESS / log Z statistics — all enqueued by
 * ONE host call, no host synchronisation inside.
 * ---------------------------------------------------------------------------------------- */
enum { FABHIP_TRANSITION_HMC = 1, FABHIP_TRANSITION_METROPOLIS = 2 };

typedef struct {
    fabhip_flow flow;
    fabhip_target target;
    int64_t B;                /* requested batch size                                        */
    int32_t M;                /* n_intermediate_distributions                                */
    const double* betas;      /* host, [M+2] (B_space, ais.py:108-129)                       */
    double alpha;
    int32_t p_target;
    int32_t transition;       /* FABHIP_TRANSITION_*                                         */
    const float* eps0;        /* [B][dim] base noise                                         */
    const float* noise_a;     /* HMC: [M][n_inner][B][dim] momenta ; Metropolis: proposals   */
    const float* noise_b;     /* HMC: [M][n_inner][B] Exp(1)       ; Metropolis: U(0,1)      */
    float* step_state;        /* HMC: epsilons[M][n_outer] ; Metropolis: noise_scalings[M][n_updates] */
    float* common_epsilon;    /* HMC only                                                    */
    const float* mass;        /* HMC only                                                    */
    int32_t n_inner;          /* n_outer (HMC) / n_updates (Metropolis)                      */
    int32_t L;
    float max_grad, target_p_accept;
    int32_t tune;
    fabhip_point point;       /* out [B] rows; first n_valid[1] rows are the result          */
    float* log_w;             /* out [B]                                                     */
    int32_t* n_valid;         /* out device int32[2]: rows after "chain init" / "chain end"  */
    float* stats;             /* out device float[16]: [0] ess_base [1] - [2] rows after init
                                 [3] ess_ais [4] log_Z [5] rows at chain end, [6..15] reserved (the init phase
                                 writes zeros): the caller need not initialise any of it                 */
    /* HMC logging slots (hmc.py:173-183, store_info), device, each may be NULL: mean acceptance probability of
     * every outer loop [n_inner] and store_info's mean distance [1], for the first (i = 1) and the last (i = M)
     * intermediate distribution.  With M = 1 only the "first" pair is written, like the reference. */
    float* p_accept_first;
    float* p_accept_last;
    float* avg_distance_first;
    float* avg_distance_last;
    /* Evaluation outputs (ais.py:152-166, generate_eval_data), each may be NULL: the chains' starting points after
     * the "chain init" filtering, base_x [B][dim], and their importance weights w.r.t. the target,
     * base_log_w [B] = log p(x0) - log q(x0) with log q as returned by the flow's sampling pass; the first
     * n_valid[0] rows are the result. */
    float* base_x;
    float* base_log_w;
    void* workspace;
    size_t workspace_bytes;
} fabhip_ais_args;

size_t fabhip_ais_workspace_bytes(int64_t B, int32_t dim, int32_t n_inner);
int fabhip_ais_run(const fabhip_ais_args* args, fabhip_stream_t stream);

/* The same call in pieces, for chains sharded over ranks with exact step-size adaptation: `phases` selects
 * FABHIP_AIS_INIT (chain initialisation, "chain init" filter, base ESS), the transitions j_begin .. j_end (1-based,
 * j_begin > j_end: none) and FABHIP_AIS_FINISH ("chain end" filter, ESS / log Z).  point / log_w / n_valid / stats are
 * in/out across the calls of one AIS run, eps0 is read by INIT only.  With `partials` != NULL (HMC, n_inner == 1,
 * j_begin == j_end) the transition leaves the step sizes alone and publishes its acceptance slab instead
 * (fabhip_hmc_args.partials); fabhip_ais_run(args) == fabhip_ais_phase(args, INIT | FINISH, 1, M, NULL).
 * Metropolis with `partials` != NULL (any j range, one call may hold the whole run): transition j leaves its noise scalings
 * alone and writes its block sums + chain count at partials + (j - 1) (n_inner nblk + 1) - the layout of
 * fabhip_metropolis_partials_floats(B, M, n_inner) - for fabhip_metropolis_adapt_gathered after the call. */
enum { FABHIP_AIS_INIT = 1, FABHIP_AIS_FINISH = 2,
       FABHIP_AIS_CONTINUE = 4 };   /* this call continues a run whose INIT phase was enqueued with the SAME workspace on the same
                                      * stream and nothing else touched the workspace since (lets the later phases keep using the
                                      * state INIT left there: the ticket of the in-kernel step-size rule).  noise_a / noise_b are
                                      * read by the transitions only: a call without transitions may pass NULL (a host can draw the
                                      * transition noise while the device runs the chain initialisation). */
int fabhip_ais_phase(const fabhip_ais_args* args, int32_t phases, int32_t j_begin, int32_t j_end, float* partials,
                     fabhip_stream_t stream);

/* SMC mode (adaptive resampling inside the call; the sampler of Del Moral et al., AIS being its special case without
 * resampling).  Before transition j = 1 .. M, with n0 = n_valid[0] chains in use:
 *   W   = fixed-point weights of log_w[:n0] (the systematic resampler's: exp_spec(log_w - max) 2^36, non-finite rows 0),
 *   ess = (sum W)^2 / (n0 sum W^2)        (integer sums, one float64 expression; sum W == 0: no resampling),
 *   ess < tau: ancestors = the systematic resampler's indices for u[j - 1] on that CDF; x, log q, log p (HMC: and both
 *              gradients) of the first n0 rows are gathered with them and every log_w[:n0] becomes
 *              max + log(sum W 2^-36 / n0), so that logsumexp(log_w) - and with it log Z - is what it was;
 *   else the step is the identity.
 * Decided and executed on the device: the launch sequence does not depend on the outcome, the host never waits.
 * `enabled` == 0 (or a NULL fabhip_smc_args): the plain call, launch for launch.  The outputs may each be NULL; transition j's
 * phase writes entry j - 1 of each.  With `partials` (sharded chains): FABHIP_ENOTSUP.  Passed as fabhip_ais_ext.smc (below).
 * `method` = FABHIP_SMC_STRATIFIED: the decision is the same, the ancestors are the stratified resampler's
 * (fabhip_resample_stratified below) for n_samples = n0 and seed = the 64 bits of the float64 u[j - 1] read as an unsigned
 * integer (u outside [0, 1): taken as 0.0, i.e. seed 0) - still one float64 per transition.  Any other value than the two
 * below: FABHIP_EINVAL. */
#define FABHIP_SMC_SYSTEMATIC 0
#define FABHIP_SMC_STRATIFIED 1
typedef struct {
    int32_t enabled;
    int32_t only_resample;    /* != 0: run the resampling steps of j_begin .. j_end WITHOUT their transitions (tests read the
                                 point between the two halves of a phase)                                                     */
    double tau;               /* threshold on ess in [1/n0, 1]; > 1: always, <= 0: never                                       */
    const double* u;          /* device [M], one uniform in [0, 1) per transition (outside the range: taken as 0); read by the
                                 transitions only - a call without transitions (FABHIP_AIS_INIT alone) may pass NULL            */
    int32_t* resampled;       /* device [M]: 1 where transition j was preceded by a resampling                                 */
    float* ess;               /* device [M]: the ess the decision saw                                                          */
    int32_t* ancestors;       /* device [M][B]: row k of the point came from row ancestors[j-1][k] (identity: no resampling)   */
    float* log_w_pre;         /* device [M][B]: log_w as the decision saw it                                                   */
    int32_t method;           /* FABHIP_SMC_SYSTEMATIC (0: what a zero-initialised struct has) or FABHIP_SMC_STRATIFIED          */
} fabhip_smc_args;

/* Defensive-mixture base distribution (fab/trainable_distributions/defensive_mixture.py; definition: tests/defensive_spec.py):
 *   log q(x) = logsumexp(log q_flow(x) + logsigmoid(l), log N(x; loc, exp(log_scale)) + logsigmoid(-l)),   l = logit[0],
 * which bounds the AIS target p^2 / q wherever the Gaussian has mass - also where the flow's float32 density underflows.
 * Gradient in closed form: r_f d log q_flow/dx + (1 - r_f) (-(x - loc) exp(-2 log_scale)), r_f = exp(a - log q) the flow's
 * responsibility (exactly 0, and the flow's gradient ignored, where log q_flow = -inf).  Chain initialisation: row i keeps the
 * flow's sample of eps0[i] iff sel[i] < sigmoid(l), else x = loc + exp(log_scale) eps0[i]; log q0 is the mixture density at x.
 * The kernels read the three parameter tensors directly (device; no packed copy, no host read).  The mode runs on the 16-chain
 * tiles at every batch size, fp32 only (FABHIP_PRECISION_FAST / the process-wide fast mode: FABHIP_ENOTSUP), not with
 * `partials` (sharded chains: FABHIP_ENOTSUP).  `enabled` == 0 (or a NULL fabhip_defensive_args): the call without the mixture,
 * launch for launch.  Composes with the SMC mode (only the point and log_w move in a resampling step); needs no workspace of its
 * own.  Passed as fabhip_ais_ext.mix (below). */
typedef struct {
    int32_t enabled;
    const float* loc;         /* device [dim]                                                                       */
    const float* log_scale;   /* device [dim]                                                                       */
    const float* logit;       /* device [1]: P(flow branch) = sigmoid(logit)                                        */
    const float* sel;         /* device [B] uniforms in [0, 1): the branch draws; read by FABHIP_AIS_INIT only      */
} fabhip_defensive_args;
/* The mixture's density alone: log_q [B] and, with grad_x != NULL, d log q / dx [B][dim] at x [B][dim] - one launch, for
 * operators stepped from the host.  `mix->sel` is not read.  `workspace`: reserved, may be NULL. */
int fabhip_defensive_log_prob(const fabhip_flow* flow, const fabhip_defensive_args* mix, const float* x, float* log_q,
                              float* grad_x, int64_t B, void* workspace, fabhip_stream_t stream);

/* Flow-proposal independence move (ABI 225; definition: tests/flow_move_spec.py).  One move at beta (coefficients `cur`):
 * x' = a fresh sample of the flow from noise_g, (x', lq', lp'[, gq', gp']) its Point, and with
 *     r(lq, lp) = (c_q lq + c_p lp) - lq       (float32, un-fused, the expression order of fabhip_anneal_log_prob)
 *     delta_i   = r(lq'_i, lp'_i) - r(lq_i, lp_i)
 * row i < n_valid takes the proposal's fields iff lq'_i and lp'_i are finite, delta_i is a number and noise_h_i > -delta_i
 * (noise_h ~ Exp(1): the Metropolis-Hastings test of an independence sampler without exp or log).  Every other row - the rows
 * at and beyond n_valid among them - is left as it is.  The move leaves pi_beta invariant: log-weights are not touched.
 * Three launches: fabhip_flow_sample into the workspace, fabhip_create_point on the proposals (gradients iff the point has
 * them; the flow's `precision` as given), the accept / commit kernel.  No host read.  n_accept [1] (int32) and p_accept [1]
 * = float32(n_accept) / float32(n_valid) (0 with n_valid == 0) may each be NULL.  workspace: 256-byte aligned,
 * fabhip_flow_move_workspace_bytes(B, dim). */
typedef struct {
    fabhip_flow flow;
    fabhip_target target;
    fabhip_point point;       /* in/out; grad_log_q / grad_log_p both NULL: a gradient-free operator's point */
    int64_t B;
    const int32_t* n_valid;   /* device scalar: rows in use (NULL -> B) */
    fabhip_anneal cur;        /* beta */
    const float* noise_g;     /* [B][dim] ~ N(0,1): the flow's base noise */
    const float* noise_h;     /* [B] ~ Exp(1) */
    float* p_accept;          /* [1] out or NULL */
    int32_t* n_accept;        /* [1] out or NULL */
    void* workspace;
    size_t workspace_bytes;
} fabhip_flow_move_args;
size_t fabhip_flow_move_workspace_bytes(int64_t B, int32_t dim);
int fabhip_flow_move(const fabhip_flow_move_args* args, fabhip_stream_t stream);

/* The moves inside the fused call: step j = 1 .. M runs [resampling step,] n_moves moves at beta_j, then transition j
 * (resample, move globally, move locally).  Steps run with smc->only_resample skip the moves.  noise_g / noise_h are read by
 * the transitions only (like noise_a / noise_b); with n_moves > 0 and transitions to run, NULL is FABHIP_EINVAL.  n_moves == 0
 * (or a NULL fabhip_flow_moves_args): the call without moves, launch for launch.  With `partials` (sharded chains) or a
 * defensive mixture: FABHIP_ENOTSUP.  Workspace: the layout of the call without moves with the proposal buffers behind it. */
typedef struct {
    int32_t n_moves;          /* k >= 0 */
    const float* noise_g;     /* device [M][k][B][dim] ~ N(0,1) */
    const float* noise_h;     /* device [M][k][B] ~ Exp(1) */
    float* p_accept_out;      /* device [M][k] acceptance fractions, or NULL; entry (j - 1, m) is written by step j's phase */
} fabhip_flow_moves_args;

/* The fused call with its optional modes (ABI 226): SMC resampling, the defensive mixture, flow-proposal moves - each described
 * at its struct above.  A NULL `ext`, a NULL member, and a member whose own switch is off (`enabled` == 0, `n_moves` == 0) all
 * mean the call without that mode, launch for launch: fabhip_ais_run(args) == fabhip_ais_run_ext(args, NULL) and
 * fabhip_ais_phase(args, ..) == fabhip_ais_phase_ext(args, NULL, ..).  Workspace: fabhip_ais_ext_workspace_bytes for the same
 * `ext` (only the switches are read; with no mode on: fabhip_ais_workspace_bytes); a mode that is on and finds its share
 * missing: FABHIP_ENOSPC.  The next mode becomes one more member here. */
typedef struct {
    const fabhip_smc_args* smc;
    const fabhip_defensive_args* mix;
    const fabhip_flow_moves_args* moves;
} fabhip_ais_ext;
size_t fabhip_ais_ext_workspace_bytes(int64_t B, int32_t dim, int32_t n_inner, const fabhip_ais_ext* ext);
int fabhip_ais_run_ext(const fabhip_ais_args* args, const fabhip_ais_ext* ext, fabhip_stream_t stream);
int fabhip_ais_phase_ext(const fabhip_ais_args* args, const fabhip_ais_ext* ext, int32_t phases, int32_t j_begin, int32_t j_end,
                         float* partials, fabhip_stream_t stream);

/* The decision alone, for samplers that step their transitions themselves (the generic plug-in path): ancestors [B] (identity
 * where nothing is resampled and beyond *n_ptr rows), resampled [1], log_w_common [1] (the value every log_w[:n0] takes when
 * resampled[0] == 1) are required; ess [1] and log_w_pre [B] may be NULL.  n_ptr NULL: all B rows.  u: device, one double.
 * method: FABHIP_SMC_SYSTEMATIC or FABHIP_SMC_STRATIFIED (fabhip_smc_args.method), anything else FABHIP_EINVAL. */
size_t fabhip_smc_workspace_bytes(int64_t B);
int fabhip_smc_decide(const float* log_w, int64_t B, const int32_t* n_ptr, double tau, const double* u, int32_t* ancestors,
                      int32_t* resampled, float* ess, float* log_w_common, float* log_w_pre, void* workspace,
                      size_t workspace_bytes, int32_t method, fabhip_stream_t stream);

/* The next temperature of an ADAPTIVE annealing schedule by ESS-decay bisection (definition: tests/adaptive_spec.py; one
 * workgroup, one launch).  With n0 = *n_ptr live rows (NULL: B; rows at and beyond n0 are never read), float32 throughout
 * unless stated:
 *     lw = log_w[:n0];  d = log_p - log_q (one float32 subtract);  s = 1 if p_target else alpha (float64)
 *     ess_of(v): W = the resampler's fixed-point weights of v (exp_spec, floor(p 2^36); a NaN / infinite entry weighs 0),
 *                S1i = sum W, S2i = sum W^2 as exact integers; S1i == 0: 0, else the float64 expression of the SMC decision,
 *                (S1 S1) / (float64(n0) S2)
 *     cand(delta) = float32(lw + float32((float64(delta) s) float64(d)))
 *     ess0 = ess_of(lw);  thr = rho ess0;  room = 1 - beta                                      (float64)
 *     room > 0 fails: 1;  ess_of(cand(room)) >= thr: 1
 *     else lo, hi = 0, room; `iters` (K) times: mid = (lo + hi) / 2; ess_of(cand(mid)) >= thr ? lo = mid : hi = mid
 *          delta = lo > 0 ? lo : hi  (the floor room / 2^K, so that every step moves);  min(beta + delta, 1)
 * out4 (device, float64): beta_next, ess0, the ESS at the chosen step (at the floor: of the floor step, below thr; without a
 * bisection: of the last candidate evaluated), evaluations + 2^16 (1 if the floor was taken).  The criterion is relative, so it
 * reads the same after a resampling step has made the weights equal.  ESS need not be monotone in delta: the bisection is the
 * definition.  beta in [0, 1], rho in (0, 1), 1 <= iters <= 60, else FABHIP_EINVAL.  No workspace. */
int fabhip_next_beta(const float* log_w, const float* log_q, const float* log_p, int64_t B, const int32_t* n_ptr, double beta,
                     double alpha, int32_t p_target, double rho, int32_t iters, double* out4, fabhip_stream_t stream);

/* SMC mode over SHARDED chains (fab_torch_amd/parallel.py: resample_across_ranks; definition: tests/smc_shard_spec.py).
 * R ranks hold b rows each, the first n_r = n_valid[0] of them live; the global live order is the ranks' live rows in rank
 * order, n0 = sum n_r, off_r = sum_{s<r} n_s.  Before a transition every rank packs its state, the host all-gathers the R
 * buffers, and every rank runs the resampling step on the gathered set: the decision is fabhip_smc_decide's kernel on the
 * n0 global log-weights (its decision, ess, ancestors and common log-weight are the single-device call's bits), and local
 * row i < n_r becomes global row ancestors[off_r + i].  Counts do not change; rows at and beyond n_r are untouched.
 *
 * fabhip_smc_shard_pack: ONE launch writes send [b + 1][RW], RW = 3 dim + 4: row i < b = x | grad log q | grad log p |
 * log q, log p, log w, 0 (the gradient slots are left unwritten when point->grad_log_q == NULL), row b = n_r (an int32 bit
 * pattern in its first word, read from the device's n_valid[0]; the rest 0). */
int fabhip_smc_shard_pack(const fabhip_point* point, const float* log_w, const int32_t* n_valid, int64_t b, int32_t dim,
                          float* send, fabhip_stream_t stream);
/* fabhip_smc_shard_resample: gathered [R][b + 1][RW] (the R send buffers in rank order), this rank's state in / out.  Three
 * launches whatever the decision (the kernels read the device flag; the host never waits): counts -> offsets and the global
 * log-weight column, the decision, the fetch of this rank's ancestors out of `gathered` (one wave per row; 16-byte accesses
 * when dim % 4 == 0 and the arrays are 16-byte aligned).  u: device, one double.  Outputs, each may be NULL: resampled [1],
 * ess [1], ancestors [R b] (global live indices; the identity where nothing is resampled and beyond n0), log_w_pre [R b]
 * (the n0 global log-weights the decision saw, -inf behind them).  R > 64: FABHIP_ENOTSUP (the offsets are one wave's
 * prefix).  workspace: 256-byte aligned, fabhip_smc_shard_workspace_bytes(R, b) (0 for an unsupported R). */
size_t fabhip_smc_shard_workspace_bytes(int32_t R, int64_t b);
int fabhip_smc_shard_resample(const float* gathered, int32_t R, int32_t rank, int64_t b, int32_t dim, double tau, const double* u,
                              const fabhip_point* point, float* log_w, const int32_t* n_valid, int32_t* resampled, float* ess,
                              int32_t* ancestors, float* log_w_pre, void* workspace, size_t workspace_bytes,
                              fabhip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same with the RQ-spline flow (fabhip_spline_*) as base distribution
 * ---------------------------------------------------------------------------------------- */
/* One HMC transition (hmc.py:129-160: n_outer x (momentum refresh, L leapfrogs, Metropolis test, in-place commit,
 * step-size adaptation) + the AIS log-weight increment when log_w != NULL) with the SPLINE flow as base distribution and a
 * native target, enqueued by one host call: per leapfrog the generic element-wise kernels, the one-launch spline density +
 * gradient kernel and the target kernel.  Same argument meaning as fabhip_hmc_args; `n_valid` (device scalar, may be
 * NULL) = rows in use.  workspace: fabhip_spline_hmc_workspace_bytes. */
typedef struct {
    fabhip_spline_flow flow;
    fabhip_target target;
    fabhip_point point;     /* in/out */
    int64_t B;
    const int32_t* n_valid;
    fabhip_anneal cur, next;
    float* log_w;
    const float* noise_p;   /* [n_outer][B][dim] */
    const float* noise_e;   /* [n_outer][B]      */
    float* epsilons;        /* -> epsilons[i-1][0..n_outer) */
    float* common_epsilon;
    const float* mass;
    int32_t n_outer, L;
    float max_grad, target_p_accept;
    int32_t tune;
    float* p_accept;        /* [n_outer] or NULL */
    float* avg_distance;    /* [1] or NULL       */
    void* workspace;
    size_t workspace_bytes;
} fabhip_spline_hmc_args;
size_t fabhip_spline_hmc_workspace_bytes(int32_t dim, int32_t n_layers, int32_t hidden, int64_t B);
int fabhip_spline_hmc_transition(const fabhip_spline_hmc_args* args, fabhip_stream_t stream);

/* AnnealedImportanceSampler.sample_and_log_weights (ais.py:53-105) with the spline flow as base distribution, a native
 * target and HMC transitions - the spline family's fabhip_ais_run: flow sample, point creation (log q re-evaluated
 * through log_prob, base.py:65-68), initial log-weights, "chain init" filter, base ESS, M transitions, "chain end"
 * filter, ESS / log Z, enqueued by ONE host call without host synchronisation.  u0 / eps0 [B][dim]: the uniforms /
 * normals of the flow's base sample (fabhip_spline_sample); everything else as in fabhip_ais_args. */
typedef struct {
    fabhip_spline_flow flow;
    fabhip_target target;
    int64_t B;
    int32_t M;
    const double* betas;
    double alpha;
    int32_t p_target;
    const float* u0;
    const float* eps0;
    const float* noise_p;   /* [M][n_outer][B][dim] */
    const float* noise_e;   /* [M][n_outer][B]      */
    float* epsilons;        /* [M][n_outer]         */
    float* common_epsilon;
    const float* mass;
    int32_t n_outer, L;
    float max_grad, target_p_accept;
    int32_t tune;
    fabhip_point point;     /* out */
    float* log_w;
    int32_t* n_valid;       /* out device int32[2] */
    float* stats;           /* out device float[16], layout of fabhip_ais_args.stats */
    float* p_accept_first;
    float* p_accept_last;
    float* avg_distance_first;
    float* avg_distance_last;
    float* base_x;          /* optional, see fabhip_ais_args */
    float* base_log_w;
    void* workspace;
    size_t workspace_bytes;
} fabhip_spline_ais_args;
size_t fabhip_spline_ais_workspace_bytes(int32_t dim, int32_t n_layers, int32_t hidden, int64_t B);
int fabhip_spline_ais_run(const fabhip_spline_ais_args* args, fabhip_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * ESS / log Z  (fab/utils/numerical.py:18-23, fab/sampling_methods/ais.py:80-86)
 * out[0] = normalised ESS of log_w[0..n), out[1] = logsumexp(log_w) - log(n_norm), out[2] = n used.
 * n is read from n_ptr (device) when n_ptr != NULL; nothing at or beyond it is read.
 * Special values as float64 torch gives them: a -inf weighs 0 and counts in n; a NaN makes ESS and
 * log Z NaN; a +inf makes the ESS NaN (softmax) and log Z +inf (logsumexp); all -inf: ESS NaN, log Z -inf.
 * n == 0 (the tail of a chain phase in which every row died - the reference raises there, ais.py:190-213,
 * so this lies outside the oracle's domain): ESS NaN, log Z -inf, out[2] = 0; the compaction moves nothing
 * and reports a count of 0.
 * ---------------------------------------------------------------------------------------- */
size_t fabhip_ess_workspace_bytes(int64_t n);
int fabhip_ess_logz(const float* log_w, int64_t n, const int32_t* n_ptr, double n_norm, float* out,
                    void* workspace, size_t workspace_bytes, fabhip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Resampling  (fab/sampling_methods/base.py:121-124 -> torch.multinomial)
 * ---------------------------------------------------------------------------------------- */
/* Bit-exact restatement of torch's CPU multinomial-with-replacement given probs[n] (float32) and
 * the float64 uniforms it consumed: sequential fp32 cumsum, /sum, last bucket = 1, lower bound. */
size_t fabhip_multinomial_torch_workspace_bytes(int64_t n);
int fabhip_multinomial_torch(const float* probs, int64_t n, const double* u, int64_t n_samples,
                             int64_t* idx, void* workspace, size_t workspace_bytes,
                             fabhip_stream_t stream);

/* Scalable fixed-point CDF resamplers from log-weights (any n): p_i = exp_spec(w_i - max w) (a specified fp32
 * exponential, oracle/numerical.py), q_i = floor(p_i 2^36), C = inclusive integer prefix sum.
 *   multinomial: idx_k = first j with C_j > floor(u_k * C_total)                (decoupled look-back scan + search)
 *   systematic : idx_k = first j with C_j > floor((k + u0) * (C_total / n_samples))
 *                fused: wave-tile sums -> tile prefix -> every tile emits the strata that fall inside its CDF range;
 *                the CDF never touches HBM (12n + 8 n_samples bytes of traffic).
 * Non-finite rows weigh 0; C_total == 0 (every weight dead): every index of both samplers is n - 1. */
size_t fabhip_resample_workspace_bytes(int64_t n);
/* The fixed-point inclusive CDF C[0..n) (uint64) of log-weights, built in the workspace by ONE decoupled-look-back scan
 * pass (4n bytes read, 8n written) after a max pass (4n read); *cdf_out (host pointer-to-device-pointer, may be
 * NULL) receives its device address inside the workspace.  reuse_max != 0 skips the max pass and uses the maximum a
 * previous call on the same log_w left in this workspace (measurement of the scan pass alone). */
int fabhip_fixed_cdf(const float* log_w, int64_t n, int32_t reuse_max, const uint64_t** cdf_out, void* workspace,
                     size_t workspace_bytes, fabhip_stream_t stream);
int fabhip_resample_multinomial(const float* log_w, int64_t n, const double* u, int64_t n_samples,
                                int64_t* idx, void* workspace, size_t workspace_bytes,
                                fabhip_stream_t stream);
int fabhip_resample_systematic(const float* log_w, int64_t n, double u0, int64_t n_samples, int64_t* idx,
                               void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
/* Seeded streaming multinomial resampler: multinomial resampling from (log_w, seed) alone - no tensor of uniforms, no CDF and
 * no array of thresholds in HBM.  The definition is the project's own (tests/resample_stream_spec.py restates it; the device
 * follows it bit for bit on any launch geometry):
 *   W, C, total: the fixed-point weights and CDF above (non-finite rows weigh 0); total == 0: every index is n - 1.
 *   spacing i = 0 .. n_samples:  z = seed + (i + 1) * 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ z >> 27) * 0x94D049BB133111EB;  r = z ^ z >> 31   (64-bit, the splitmix64 finaliser);  y = (r >> 32) | 1,
 *     lz = clz32(y), f = float(((y << lz) mod 2^32) >> 8) * 2^-23 in [1, 2), u_i = f * 2^-(lz + 1) in (0, 1);
 *     e_i = max(1, K * 186065279 - rint(p(g - 1) * 2^28)),  g = f >= 1.41421354f ? f / 2 : f,  K = lz + 1 - (f >= 1.41421354f),
 *     p(t) = t (1 + t (c7 + .. t c0)) a float32 Horner form of ln(1 + t) with individually rounded operations and the
 *     coefficients 0.08743945509195328, -0.14377330243587494, 0.14949095249176025, -0.16560696065425873, 0.19956977665424347,
 *     -0.2500215470790863, 0.3333418369293213, -0.49999988079071045, 1 (highest first): e_i is -ln(u_i) with 28 fractional
 *     bits, |e_i 2^-28 + ln u_i| <= 1.3e-7, e_i < 2^33.
 *   G_k = e_0 + .. + e_k (exact); G_k / G_ns, k < n_samples, are distributed as the SORTED values of n_samples iid uniforms.
 *   sorted draw k:  idx_k = first j with C_j * G_ns > G_k * total   (128-bit products; non-decreasing in k).
 *   order = FABHIP_ORDER_SORTED returns idx (what the systematic resampler returns: all a row gather needs);
 *   order = FABHIP_ORDER_SHUFFLED returns out[k] = idx[pi(k)], pi the Feistel / cycle-walking bijection of [0, n_samples) that
 *   fabhip_topk's random order uses, its four round keys the low 32 bits of r for i = 2^40 + j: an exchangeable multinomial
 *   sample, as torch.multinomial gives.
 * n_samples <= FABHIP_STREAM_MAX_SAMPLES keeps G_ns < 2^62; more is FABHIP_EINVAL, like n < 1, n_samples < 1, an unknown
 * order, a NULL pointer or a workspace that is not 256-byte aligned; a workspace smaller than
 * fabhip_resample_stream_workspace_bytes(n, n_samples) (0 for arguments the call refuses) is FABHIP_ENOSPC.  All of it is
 * checked before any launch and without touching a device.  The caller owns log_w [n], idx [n_samples] and the workspace
 * (device memory); nothing is allocated, nothing synchronises, every launch goes to `stream`.
 * Traffic, order = sorted: log_w three times (maximum, tile sums, merge), 8 n_samples bytes of indices, and per 1024
 * weights / 1024 draws a few 8-byte prefix words - the systematic call's 12 n + 8 n_samples. */
#define FABHIP_ORDER_SORTED 0
#define FABHIP_ORDER_SHUFFLED 1
#define FABHIP_STREAM_MAX_SAMPLES ((int64_t)((1ll << 29) - 1))
size_t fabhip_resample_stream_workspace_bytes(int64_t n, int64_t n_samples);
int fabhip_resample_multinomial_stream(const float* log_w, int64_t n, uint64_t seed, int64_t n_samples, int32_t order,
                                       int64_t* idx, void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
/* Seeded stratified resampler: one independent uniform per stratum (the systematic resampler draws one for all of them), from
 * (log_w, seed) alone.  Unbiased, every count within two of n_samples W_j / total, variance never above multinomial
 * resampling's and - unlike the systematic resampler's - independent of the order of the particles.  The definition is the
 * project's own (tests/resample_stratified_spec.py restates it; the device follows it bit for bit on any launch geometry):
 *   W, C, total: the fixed-point weights and CDF above (non-finite rows weigh 0); total == 0: every index is n - 1.
 *   F = 62 - bit_length(total), S = floor(total 2^F / n_samples): the systematic resampler's stratum map.
 *   stratum k = 0 .. n_samples - 1:  h_k = the splitmix64 finaliser r above for i = k (the counter is the stratum number),
 *     U_k = (h_k * S) >> 64, the high half of the 128-bit product, in [0, S - 1];  t_k = (k S + U_k) >> F;
 *     idx_k = first j with C_j > t_k   (k S + U_k < 2^62: 64-bit integers throughout; non-decreasing in k).
 *   Inverse evaluated per CDF value (no CDF and no thresholds in HBM): with B = C_j << F and q = min(floor(B / S), n_samples),
 *     K(C_j) = q + [q < n_samples and q S + U_q < B], weight j owns the strata [K(C_{j-1}), K(C_j)).
 *   order = FABHIP_ORDER_SORTED returns idx; FABHIP_ORDER_SHUFFLED returns out[k] = idx[pi(k)], pi the keyed bijection of the
 *   streaming multinomial resampler above (same keys: the low 32 bits of r for i = 2^40 + j).
 * Limits: n >= 1, 1 <= n_samples <= FABHIP_STRATIFIED_MAX_SAMPLES = 2^31 - 3.  FABHIP_EINVAL for n < 1, n_samples < 1, n_samples
 * beyond the limit, an unknown order, a NULL pointer or a workspace that is not 256-byte aligned; FABHIP_ENOSPC for a workspace
 * smaller than fabhip_resample_stratified_workspace_bytes(n, n_samples) (0 for arguments the call refuses).  All of it is
 * checked before any launch and without touching a device.  The caller owns log_w [n], idx [n_samples] and the workspace
 * (device memory); nothing is allocated, nothing synchronises, every launch goes to `stream`.
 * Launches: maximum (2), wave-tile sums, block prefix + stratum map, emit, grid-wide fill of runs >= 32768 (n_samples >= 32768
 * only), shuffle (order = shuffled only).  Traffic, order = sorted: the systematic call's 12 n + 8 n_samples bytes; one hash per
 * weight, none per draw. */
#define FABHIP_STRATIFIED_MAX_SAMPLES ((int64_t)((1ll << 31) - 3))
size_t fabhip_resample_stratified_workspace_bytes(int64_t n, int64_t n_samples);
int fabhip_resample_stratified(const float* log_w, int64_t n, uint64_t seed, int64_t n_samples, int32_t order, int64_t* idx,
                               void* workspace, size_t workspace_bytes, fabhip_stream_t stream);
/* dst[k][:] = src[idx[k]][:]  (Point.__getitem__ / tensor indexing used by resample) */
int fabhip_gather_rows(const float* src, const int64_t* idx, float* dst, int64_t n_out, int64_t row_len,
                       fabhip_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Top-k selection — the `torch.topk(gumbel + logits, n)` of the prioritised buffer's sampling without
 * replacement (fab/utils/prioritised_replay_buffer.py:10-17, called from :100-110 with n = n_batches * batch).
 * sorted = 0: idx_out = the indices of the k largest keys in ascending index order (ties at the threshold: lowest
 * indices first) — all the buffer needs, it permutes them randomly afterwards; any k <= n.
 * sorted = 1: descending key order, ties by ascending index (torch.topk with sorted=True up to its unspecified tie
 * order), k <= 16384 (one LDS-resident sort, else FABHIP_ENOTSUP); key_out (optional) = those keys.
 * NaN ranks above +inf as in torch; n < 2^32.
 * ---------------------------------------------------------------------------------------- */
size_t fabhip_topk_workspace_bytes(int64_t n, int64_t k);
int fabhip_topk(const float* keys, int64_t n, int64_t k, int32_t sorted, int64_t* idx_out, float* key_out,
                void* workspace, size_t workspace_bytes, fabhip_stream_t stream);

/* Diagnostics (development only): with FABHIP_TIMELINE=1 in the environment fabhip_flow_log_prob records
 * s_memtime stamps at the stage boundaries of one forward and one backward layer of workgroup 0;
 * this call copies the first n (<= 64) stamps to the host (synchronises). */
int fabhip_debug_timeline(int64_t* host_out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* FABHIP_H */
