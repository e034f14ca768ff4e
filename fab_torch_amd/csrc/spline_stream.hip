// Spline coupling flow: the one-launch density (+ gradient) kernel on 4x4x1 MFMA weight streams, k_spline_logprob_r8 (spline_r8.h:
// hidden widths padded to 256), its tile-shape choice, the one-launch leapfrog of the fused spline transition built on it - and,
// because the choice between this kernel, the 16x16x4 kernel and the staged pass (both spline_tile16.hip) is made here, the
// density entry point fabhip_spline_log_prob and the workspace size.
#include "flow_device.h"
#include "target_device.h"
#include "stream_r8.h"
#include "launch.h"
#include <stdlib.h>

#pragma clang fp contract(off)

#include "spline_device.h"
#include "spline_r8.h"
#include "spline_host.h"

namespace fab {

// dev-only stage timeline (FABHIP_TIMELINE=1): s_memtime stamps of workgroup 0 in layer 1 of k_spline_logprob / k_spline_logprob_r8
static long long* g_sp_timeline = nullptr;
long long* sp_timeline(hipStream_t st) {
    if (!option(FABHIP_OPT_TIMELINE)) return nullptr;
    if (!g_sp_timeline && hipMalloc((void**)&g_sp_timeline, 32 * 8) != hipSuccess) return nullptr;
    hipMemsetAsync(g_sp_timeline, 0, 32 * 8, st);
    return g_sp_timeline;
}

// 8-chain tiles (spline_r8.h): hidden width padded to 256, fp32 path.  FABHIP_OPT_TILE_SHAPE 16 / 8 (or 4) forces a shape;
// otherwise 8-chain tiles whenever 16-chain tiles would leave CUs without a workgroup.
// The 4x4x1 stream kernels (spline_r8.h; hidden width padded to 256, fp32 path): 4 / 8 chains per workgroup while that leaves
// no CU with more than one workgroup (the kernel's registers allow no second one: 1024 / 2048 chains on MI355X), 16 above.
// FABHIP_OPT_TILE_SHAPE 4 / 8 / 16 forces the tile; FABHIP_OPT_SPLINE_MFMA = 16 selects the 16x16x4 kernel
// (k_spline_logprob: the only one for other widths and for fast mode).  Returns row blocks (0: not this kernel).
static int r8_row_blocks(const SplineDims& f, long B, int fast, bool grad) {
    if (f.NTWM != 4 || !f.o_r8 || option(FABHIP_OPT_SPLINE_MFMA) == 16) return 0;
    const int sel = option(FABHIP_OPT_TILE_SHAPE);
    int rb = sel == 16 ? 4 : (sel == 8 ? 2 : (sel == 4 ? 1 : (B <= 4L * cu_count() ? 1 : (B <= 8L * cu_count() ? 2 : 4))));
    // fast mode is a PERMISSION to use bf16: up to 8 chains per CU the fp32 stream kernel is the faster one (cfg 3: 0.39 ms
    // against 0.45 for the bf16 16-chain kernel), so fast-mode calls take it too; above, the bf16 kernel (0.68 against 1.03 ms)
    if (fast && rb == 4) return 0;
    // the LDS plan grows with the layer count (ReLU ballots) and the output chunks: deep / wide flows fall back to the smaller
    // tile, then to the 16x16x4 kernel (whose ballots live in the workspace)
    if (rb == 4 && (size_t)make_s8_lds(f, grad, 16).total * 4 > 160 * 1024) rb = 2;
    if (rb == 2 && (size_t)make_s8_lds(f, grad, 8).total * 4 > 160 * 1024) rb = 1;
    if (rb == 1 && (size_t)make_s8_lds(f, grad, 4).total * 4 > 160 * 1024) rb = 0;
    return rb;
}

template <int NCH, int RB, bool TRIM = false>
static int launch_logprob_r8(const SplineDims& f, const float* packed, const float* x, float* log_q, float* grad_x, long B,
                             float* Zsave, float* Psave, hipStream_t st, const SplineLeapDev& lp) {
    const dim3 grid((unsigned)ceil_div((int)B, 4 * RB)), block(NTHREADS);
    const S8Lds l = make_s8_lds(f, grad_x != nullptr, 4 * RB);
    const size_t bytes = (size_t)l.total * 4;
    long long* tl = sp_timeline(st);                       // (enqueues its memset: in front of the kernel)
    if (grad_x)
        return launch_lds(k_spline_logprob_r8<NCH, RB, true, TRIM>, grid, block, bytes, st, f, l, packed, x, log_q, grad_x, B, Zsave,
                          Psave, tl, lp);
    return launch_lds(k_spline_logprob_r8<NCH, RB, false, TRIM>, grid, block, bytes, st, f, l, packed, x, log_q, grad_x, B, Zsave,
                      Psave, tl, SplineLeapDev{});
}

template <int RB>
static int launch_logprob_r8_nch(const SplineDims& f, const float* packed, const float* x, float* log_q, float* grad_x, long B,
                                 float* Zsave, float* Psave, hipStream_t st, const SplineLeapDev& lp) {
    switch (f.NCH) {
        case 1: return launch_logprob_r8<1, RB>(f, packed, x, log_q, grad_x, B, Zsave, Psave, st, lp);
        case 2: return f.r8_trim ? launch_logprob_r8<2, RB, true>(f, packed, x, log_q, grad_x, B, Zsave, Psave, st, lp)
                                 : launch_logprob_r8<2, RB>(f, packed, x, log_q, grad_x, B, Zsave, Psave, st, lp);
        case 3: return launch_logprob_r8<3, RB>(f, packed, x, log_q, grad_x, B, Zsave, Psave, st, lp);
        case 4: return launch_logprob_r8<4, RB>(f, packed, x, log_q, grad_x, B, Zsave, Psave, st, lp);
        default: return FABHIP_ENOTSUP;
    }
}

// the stream kernel on `rb` row blocks (r8_row_blocks: 1 / 2 / 4 = 4 / 8 / 16 chains per workgroup); lp.XP: the leapfrog around it
static int launch_logprob_r8_rb(int rb, const SplineDims& f, const float* packed, const float* x, float* log_q, float* grad_x, long B,
                                const SplineWs& w, hipStream_t st, const SplineLeapDev& lp = SplineLeapDev{}) {
    switch (rb) {
        case 1: return launch_logprob_r8_nch<1>(f, packed, x, log_q, grad_x, B, w.Z, w.P, st, lp);
        case 2: return launch_logprob_r8_nch<2>(f, packed, x, log_q, grad_x, B, w.Z, w.P, st, lp);
        case 4: return launch_logprob_r8_nch<4>(f, packed, x, log_q, grad_x, B, w.Z, w.P, st, lp);
        default: return FABHIP_ENOTSUP;
    }
}

// launch.h: the outer step's begin / accept / step-size rule inside the leapfrog launches - where the one-launch leapfrog
// applies, the switch is on and the last wave's 2 nblk block sums fit the conditioner-output tile it uses as scratch
size_t spline_fold_scratch_floats(int64_t B) { return (size_t)32 * ((B + 15) / 16) + 64; }
// THE applicability test of the one-launch leapfrog, shared by the query below and by spline_log_prob_leap itself (a precondition
// added to one of them only would turn the caller's fallback into a failure half-way through an outer step): chains per
// workgroup / 8 of the kernel that would run, 0 where it does not apply
static int spline_leap_row_blocks(const fabhip_spline_flow* flow, int64_t B, SplineDims* dims) {
    if (!flow || !flow->packed || B < 1 || !option(FABHIP_OPT_SPLINE_LEAP) || option(FABHIP_OPT_SPLINE_STAGED)) return 0;
    if (check_spline_shape(flow->dim, flow->n_layers, flow->hidden) != FABHIP_OK) return 0;
    *dims = make_spline_dims(flow->dim, flow->n_layers, flow->hidden);
    return r8_row_blocks(*dims, (long)B, resolve_fast(flow->precision), true);
}
bool spline_leap_fold_supported(const fabhip_spline_flow* flow, int64_t B) {
    SplineDims f;
    const int rb = spline_leap_row_blocks(flow, B, &f);
    if (rb == 0 || !option(FABHIP_OPT_ADAPT_FOLD)) return false;
    const S8Lds l = make_s8_lds(f, true, 4 * rb);
    return 2 * ((B + 15) / 16) <= (int64_t)(4 * rb) * l.PS;
}

// launch.h: one leapfrog of the spline family in one launch
int spline_log_prob_leap(const fabhip_spline_flow* flow, const SplineLeap& a, float* log_q, float* grad_x, int64_t B,
                         void* workspace, size_t workspace_bytes, hipStream_t st) {
    if (!flow || !flow->packed || !a.XP || !a.x_out || !a.P || !a.GU || !log_q || !grad_x || !workspace || B < 0) return FABHIP_EINVAL;
    FAB_TRY(check_spline_shape(flow->dim, flow->n_layers, flow->hidden));
    FAB_TRY(check_target(&a.tg, flow->dim));
    if (B == 0) return FABHIP_OK;
    SplineDims f;
    const int rb = spline_leap_row_blocks(flow, B, &f);
    if (rb == 0) return FABHIP_ENOTSUP;
    if (workspace_bytes < fabhip_spline_workspace_bytes(flow->dim, flow->n_layers, flow->hidden, B, 1)) return FABHIP_ENOSPC;
    SplineLeapDev d;
    d.XP = a.XP; d.x_out = a.x_out; d.P = a.P; d.GU = a.GU; d.eps_ptr = a.eps_ptr; d.ceps_ptr = a.ceps_ptr; d.mass = a.mass; d.c = a.c;
    d.max_grad = a.max_grad; d.tg = make_target_dev(a.tg); d.prop_lp = a.prop_lp; d.prop_gp = a.prop_gp;
    d.fold = a.fold;
    if (d.fold.flags && !spline_leap_fold_supported(flow, B)) return FABHIP_EINVAL;   // (the caller asks first)
    return launch_logprob_r8_rb(rb, f, flow->packed, a.XP, log_q, grad_x, (long)B, carve_spline_ws(workspace, f, (long)B, true), st, d);
}

int spline_log_prob_impl(const fabhip_spline_flow* flow, const float* x, float* log_q, float* grad_x, int64_t B, float* tape,
                         void* workspace, size_t workspace_bytes, hipStream_t st) {
    if (!flow || !flow->packed || !x || !log_q || !workspace || B < 0) return FABHIP_EINVAL;
    FAB_TRY(check_spline_shape(flow->dim, flow->n_layers, flow->hidden));
    if (B == 0) return FABHIP_OK;
    if (workspace_bytes < fabhip_spline_workspace_bytes(flow->dim, flow->n_layers, flow->hidden, B, grad_x != nullptr))
        return FABHIP_ENOSPC;
    const SplineDims f = make_spline_dims(flow->dim, flow->n_layers, flow->hidden);
    const SplineWs w = carve_spline_ws(workspace, f, (long)B, grad_x != nullptr);
    const float* pk = flow->packed;
    if (tape || option(FABHIP_OPT_SPLINE_STAGED))        // the staged kernels: tape, debugging
        return spline_log_prob_staged(f, pk, x, log_q, grad_x, (long)B, tape, w, st);
    const int fast = resolve_fast(flow->precision);
    const int rb = r8_row_blocks(f, (long)B, fast, grad_x != nullptr);
    if (rb) return launch_logprob_r8_rb(rb, f, pk, x, log_q, grad_x, (long)B, w, st);
    return spline_logprob_t16(f, pk, x, log_q, grad_x, (long)B, w, fast, st);
}

}  // namespace fab

using namespace fab;

extern "C" {

int fabhip_debug_spline_timeline(int64_t* host_out, int32_t n) {
    if (!g_sp_timeline || !host_out || n < 1 || n > 32) return FABHIP_EINVAL;
    return hipMemcpy(host_out, g_sp_timeline, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess ? FABHIP_OK : FABHIP_ELAUNCH;
}

size_t fabhip_spline_workspace_bytes(int32_t dim, int32_t n_layers, int32_t hidden, int64_t B, int32_t with_grad) {
    if (check_spline_shape(dim, n_layers, hidden) != FABHIP_OK) return 0;
    return carve_spline_ws(nullptr, make_spline_dims(dim, n_layers, hidden), (long)B, with_grad != 0).bytes;
}

int fabhip_spline_log_prob(const fabhip_spline_flow* flow, const float* x, float* log_q, float* grad_x, int64_t B,
                           void* workspace, size_t workspace_bytes, fabhip_stream_t stream) {
    return spline_log_prob_impl(flow, x, log_q, grad_x, B, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
