// AIS inner loop on 16-chain tiles: point creation, the Metropolis transition and its noise-scaling rule kernels
// (chain initialisation and the HMC transition: ais_tile16.hip).
#include "flow_device.h"
#include "target_device.h"
#include "launch.h"
#include "defensive_device.h"

#pragma clang fp contract(off)   // keep a*b+c un-fused in the elementwise code, like the eager CPU reference

#include "ais_device.h"
#include "ais_host.h"
#include "ais_tile16.h"

namespace fab {

// ------------------------------------------------------------------------------------------------
// create_point: log q (+grad), log p (+grad) at point.x      (fab/sampling_methods/base.py:59-72)
// ------------------------------------------------------------------------------------------------
// MIX: the defensive mixture's density (+ gradient) alone, for fabhip_defensive_log_prob: no target is evaluated, pt.lp / pt.gp
// are not written (the fused call creates its points in ais_init_body / hmc_step_body / metropolis_body).
template <int NTWM, bool GRAD, bool FAST, bool MIX = false>
__device__ __forceinline__ void create_point_body(const FlowDims& f, const FlowLds& l, const ExtraLds& x,
                                                  const float* __restrict__ packed, const TargetDev& tg, const PointDev& pt,
                                                  long B, float* lds, const MixDev& mx = MixDev{}) {
    Tid t;
    const int D = f.D;
    const long row0 = (long)blockIdx.x * ROWS;
    float* XP = lds + x.o_XP;
    float* GP = lds + x.o_GP;
    float* MP = lds + x.total;                               // MIX: the staged mixture parameters, behind the plan
    if constexpr (MIX) mix_stage(mx, D, MP, t);
    zero_dp(l, lds, t);
    for (int e = t.tid; e < ROWS * D; e += NTHREADS) {
        const long g = row0 + e / D;
        XP[e] = g < B ? pt.x[g * D + e % D] : 0.f;
    }
    __syncthreads();
    load_state_to_u0(l, D, lds, XP, t);
    __syncthreads();
    int goff = 0;
    float lq = flow_log_prob_tile<NTWM, GRAD, false, FAST>(f, l, packed, lds, t, &goff);
    if constexpr (MIX) {
        lq = mix_tile<GRAD>(MP, D, XP, D, lds + goff, l.DS, lq, t);
        const long g = row0 + t.row;
        if (g < B) {
            if (t.c == 0) pt.lq[g] = lq;
            if (GRAD) for (int j = t.c; j < D; j += 16) pt.gq[g * D + j] = lds[goff + t.row * l.DS + j];
        }
        return;
    }
    const float lp = target_tile<GRAD>(tg, XP, D, GP, D, t);
    const long g = row0 + t.row;
    if (g < B) {
        if (t.c == 0) { pt.lq[g] = lq; pt.lp[g] = lp; }
        if (GRAD) {
            for (int j = t.c; j < D; j += 16) {
                pt.gq[g * D + j] = lds[goff + t.row * l.DS + j];
                pt.gp[g * D + j] = GP[t.row * D + j];
            }
        }
    }
}

template <int NTWM, bool GRAD>
__global__ __launch_bounds__(NTHREADS) void k_create_point(FlowDims f, FlowLds l, ExtraLds x, const float* __restrict__ packed,
                                                           TargetDev tg, PointDev pt, long B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    create_point_body<NTWM, GRAD, false>(f, l, x, packed, tg, pt, B, lds);
}
template <int NTWM, bool GRAD>
__global__ __launch_bounds__(NTHREADS) void k_create_point_mix(FlowDims f, FlowLds l, ExtraLds x, const float* __restrict__ packed,
                                                               PointDev pt, long B, MixDev mx) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    create_point_body<NTWM, GRAD, false, true>(f, l, x, packed, TargetDev{}, pt, B, lds, mx);
}
// fast mode (bf16 W x W GEMMs, flow_device.h): same kernel, not the parity path
template <int NTWM, bool GRAD>
__global__ __launch_bounds__(NTHREADS) void k_create_point_fast(FlowDims f, FlowLds l, ExtraLds x,
                                                                const float* __restrict__ packed, TargetDev tg, PointDev pt,
                                                                long B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    create_point_body<NTWM, GRAD, true>(f, l, x, packed, tg, pt, B, lds);
}

// ------------------------------------------------------------------------------------------------
// Metropolis transition: all n_updates for 16 chains per workgroup (metropolis.py:51-74; arguments: ais_device.h, MetK).
// ------------------------------------------------------------------------------------------------
template <int NTWM, bool MIX>
__device__ __forceinline__ void metropolis_body(const FlowDims& f, const FlowLds& l, const ExtraLds& x,
                                                const float* __restrict__ packed, const TargetDev& tg, const MetK& a,
                                                float* lds, const MixDev& mx = MixDev{}) {
    Tid t;
    const int D = f.D;
    const long nv = a.n_valid ? (long)*a.n_valid : a.B;
    const long row0 = (long)blockIdx.x * ROWS;
    if (row0 >= nv) {
        for (int n = t.tid; n < a.n_updates; n += NTHREADS) a.part_acc[(long)n * a.nblk + blockIdx.x] = 0.f;
        return;
    }
    float* XC = lds + x.o_XP;        // current positions
    float* XN = lds + x.o_P;         // proposals
    float* GP = lds + x.o_GP;
    float* ROWB = lds + x.o_ROW;
    const long g = row0 + t.row;
    const bool active = g < nv;
    if constexpr (MIX) mix_stage(mx, D, lds + x.total, t);
    zero_dp(l, lds, t);
    for (int j = t.c; j < D; j += 16) XC[t.row * D + j] = active ? a.cur.x[g * D + j] : 0.f;
    float lq_c = 0.f, lp_c = 0.f;
    if (active) { lq_c = a.cur.lq[g]; lp_c = a.cur.lp[g]; }
    const float prev_lp = a.c.c_q * lq_c + a.c.c_p * lp_c;     // computed once, never refreshed (metropolis.py:53)
    bool changed = false;
    for (int n = 0; n < a.n_updates; ++n) {
        const float sc = a.scalings[n];
        for (int j = t.c; j < D; j += 16) {
            const float nz = active ? a.noise_x[((long)n * a.B + g) * D + j] : 0.f;
            XN[t.row * D + j] = XC[t.row * D + j] + nz * sc;
        }
        __syncthreads();
        load_state_to_u0(l, D, lds, XN, t);
        __syncthreads();
        int goff;
        float lq = flow_log_prob_tile<NTWM, false>(f, l, packed, lds, t, &goff);
        if constexpr (MIX) lq = mix_tile<false>(lds + x.total, D, XN, D, nullptr, 0, lq, t);
        const float lp = target_tile<false>(tg, XN, D, GP, D, t);
        float acc = expf((a.c.c_q * lq + a.c.c_p * lp) - prev_lp);
        if (!isfinite(acc)) acc = 0.f;                          // nan_to_num(nan=0, posinf=0, neginf=0)
        bool accept = false;
        if (active) accept = acc > a.noise_u[(long)n * a.B + g];
        if (accept) {
            for (int j = t.c; j < D; j += 16) XC[t.row * D + j] = XN[t.row * D + j];
            lq_c = lq; lp_c = lp; changed = true;
        }
        if (t.c == 0) ROWB[t.row] = active ? fminf(acc, 1.f) : 0.f;
        __syncthreads();
        if (t.tid == 0) {
            float s = 0.f;
            for (int r = 0; r < ROWS; ++r) s += ROWB[r];
            a.part_acc[n * a.nblk + blockIdx.x] = s;
        }
        __syncthreads();
    }
    if (active) {
        if (changed) {
            for (int j = t.c; j < D; j += 16) a.cur.x[g * D + j] = XC[t.row * D + j];
            if (t.c == 0) { a.cur.lq[g] = lq_c; a.cur.lp[g] = lp_c; }
        }
        if (a.log_w && t.c == 0) {
            const float num = a.nx.c_q * lq_c + a.nx.c_p * lp_c;
            const float den = a.c.c_q * lq_c + a.c.c_p * lp_c;
            a.log_w[g] = a.log_w[g] + (num - den);
        }
    }
}

template <int NTWM>
__global__ __launch_bounds__(NTHREADS) void k_metropolis(FlowDims f, FlowLds l, ExtraLds x, const float* __restrict__ packed,
                                                         TargetDev tg, MetK a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    metropolis_body<NTWM, false>(f, l, x, packed, tg, a, lds);
}
template <int NTWM>
__global__ __launch_bounds__(NTHREADS) void k_metropolis_mix(FlowDims f, FlowLds l, ExtraLds x, const float* __restrict__ packed,
                                                             TargetDev tg, MetK a, MixDev mx) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    metropolis_body<NTWM, true>(f, l, x, packed, tg, a, lds, mx);
}

__global__ void k_metropolis_adapt(const float* __restrict__ part_acc, int nblk, int n_updates, const int* n_valid,
                                   long B, float* scalings, float target_p_accept, int tune) {
    if (blockIdx.x != 0 || !tune) return;
    const long nv = n_valid ? (long)*n_valid : B;
    if (nv <= 0) return;
    for (int n = threadIdx.x; n < n_updates; n += blockDim.x) {     // any number of updates (the reference has no bound)
        float s = 0.f;
        for (int i = 0; i < nblk; ++i) s += part_acc[(long)n * nblk + i];
        const float p_accept = s / (float)nv;
        scalings[n] = (p_accept > target_p_accept) ? scalings[n] * 1.05f : scalings[n] / 1.05f;
    }
}

// Sharded chains: a Metropolis transition whose block sums went into the caller's slab instead of part_acc
// appends the number of chains in use; the rule then runs on the slabs of ALL ranks.  noise_scalings[i - 1, n] is read by
// update n of transition i only (metropolis.py:57) and adjusted right after it (:68-73): nothing later in the SAME AIS call
// reads the adjusted value, so the adjustments of all M transitions can wait for ONE gather at the end of the call.
__global__ void k_metropolis_count(const int* n_valid, long B, float* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = (float)(n_valid ? (long)*n_valid : B);
}

// thread (j, n) = transition j, update n: block sums over ranks, then blocks, in order - with shards that are multiples of 16
// chains the sequence k_metropolis_adapt adds on one device holding every chain
__global__ void k_metropolis_adapt_gathered(const float* __restrict__ slabs, int n_ranks, int nblk, int M, int n_updates,
                                            float* scalings, float target_p_accept, int tune) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M * n_updates || !tune) return;
    const int j = t / n_updates, n = t % n_updates;
    const long per_j = (long)n_updates * nblk + 1, per_rank = (long)M * per_j;
    float s = 0.f;
    long nv = 0;
    for (int r = 0; r < n_ranks; ++r) {
        const float* sl = slabs + r * per_rank + j * per_j;
        for (int i = 0; i < nblk; ++i) s += sl[n * nblk + i];
        nv += (long)sl[per_j - 1];
    }
    if (nv <= 0) return;
    const float p_accept = s / (float)nv;
    scalings[t] = (p_accept > target_p_accept) ? scalings[t] * 1.05f : scalings[t] / 1.05f;
}

// ------------------------------------------------------------------------------------------------
// host-side launchers.  `mx.on` (defensive mixture, defensive_device.h): the *_mix instantiation, fp32 only.
// ------------------------------------------------------------------------------------------------
template <int NTWM>
static int launch_create_point(const FlowDims& f, const float* packed, const TargetDev& tg, const PointDev& pt,
                               int with_grad, long B, const MixDev& mx, hipStream_t st) {
    const Lds16 p = make_lds16(f, with_grad != 0, mx);
    const dim3 grid(nblk_of(B)), block(NTHREADS);
    if (mx.on && with_grad) return launch_lds(k_create_point_mix<NTWM, true>, grid, block, p.bytes, st, f, p.l, p.x, packed, pt, B, mx);
    if (mx.on) return launch_lds(k_create_point_mix<NTWM, false>, grid, block, p.bytes, st, f, p.l, p.x, packed, pt, B, mx);
    if (with_grad && f.fast) return launch_lds(k_create_point_fast<NTWM, true>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, pt, B);
    if (with_grad) return launch_lds(k_create_point<NTWM, true>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, pt, B);
    return launch_lds(k_create_point<NTWM, false>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, pt, B);
}

template <int NTWM>
static int launch_metropolis(const FlowDims& f, const float* packed, const TargetDev& tg, const MetK& a, const MixDev& mx,
                             hipStream_t st) {
    const Lds16 p = make_lds16(f, false, mx);
    if (mx.on) return launch_lds(k_metropolis_mix<NTWM>, dim3(a.nblk), dim3(NTHREADS), p.bytes, st, f, p.l, p.x, packed, tg, a, mx);
    return launch_lds(k_metropolis<NTWM>, dim3(a.nblk), dim3(NTHREADS), p.bytes, st, f, p.l, p.x, packed, tg, a);
}

int metropolis_t16(const FlowDims& f, const float* packed, const TargetDev& tg, const MetK& a, const MixDev& mx, hipStream_t st) {
    FAB_DISPATCH_NTW(f, launch_metropolis, f, packed, tg, a, mx, st);
}

int metropolis_adapt(const float* part_acc, int nblk, int n_updates, const int* n_valid, long B, float* scalings,
                     float target_p_accept, int tune, hipStream_t st) {
    hipLaunchKernelGGL(k_metropolis_adapt, dim3(1), dim3(64), 0, st, part_acc, nblk, n_updates, n_valid, B, scalings,
                       target_p_accept, tune);
    return check_launch();
}

int metropolis_count(const int* n_valid, long B, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_metropolis_count, dim3(1), dim3(1), 0, st, n_valid, B, out);
    return check_launch();
}

}  // namespace fab

using namespace fab;

extern "C" {

int fabhip_create_point(const fabhip_flow* flow, const fabhip_target* target, const fabhip_point* point,
                        int32_t with_grad, int64_t B, fabhip_stream_t stream) {
    if (!flow || !flow->packed || !point || B < 0) return FABHIP_EINVAL;
    FAB_TRY(check_flow_shape(flow->dim, flow->n_layers, flow->width));
    FAB_TRY(check_target(target, flow->dim));
    FAB_TRY(check_point(*point, with_grad != 0));
    if (B == 0) return FABHIP_OK;
    const FlowDims f = flow_dims_of(*flow);
    FAB_DISPATCH_NTW(f, launch_create_point, f, flow->packed, make_target_dev(*target), make_point_dev(*point),
                     with_grad, (long)B, MixDev{}, (hipStream_t)stream);
}

int fabhip_defensive_log_prob(const fabhip_flow* flow, const fabhip_defensive_args* mix, const float* x, float* log_q,
                              float* grad_x, int64_t B, void* workspace, fabhip_stream_t stream) {
    (void)workspace;
    if (!flow || !flow->packed || !mix || !mix->enabled || !x || !log_q || B < 0) return FABHIP_EINVAL;
    FAB_TRY(check_flow_shape(flow->dim, flow->n_layers, flow->width));
    FAB_TRY(check_mix(mix));
    if (B == 0) return FABHIP_OK;
    const FlowDims f = flow_dims_of(*flow);
    if (f.fast) return FABHIP_ENOTSUP;                                // (no bf16 instantiation of the mixture kernels)
    const PointDev pt{const_cast<float*>(x), log_q, nullptr, grad_x, nullptr};
    FAB_DISPATCH_NTW(f, launch_create_point, f, flow->packed, TargetDev{}, pt, grad_x ? 1 : 0, (long)B, make_mix_dev(mix),
                     (hipStream_t)stream);
}

int64_t fabhip_metropolis_partials_floats(int64_t B, int32_t M, int32_t n_updates) {
    return (B < 0 || M < 1 || n_updates < 1) ? -1 : (int64_t)M * ((int64_t)n_updates * nblk_of(B) + 1);
}

int fabhip_metropolis_adapt_gathered(const float* gathered, int32_t n_ranks, int64_t B_rank, int32_t M, int32_t n_updates,
                                     float* noise_scalings, float target_p_accept, int32_t tune, fabhip_stream_t stream) {
    if (!gathered || n_ranks < 1 || B_rank < 1 || M < 1 || n_updates < 1 || !noise_scalings) return FABHIP_EINVAL;
    const int n = M * n_updates;
    hipLaunchKernelGGL(k_metropolis_adapt_gathered, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, gathered, n_ranks,
                       nblk_of(B_rank), M, n_updates, noise_scalings, target_p_accept, tune);
    return check_launch();
}

}  // extern "C"
