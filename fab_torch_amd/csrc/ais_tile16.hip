// AIS inner loop on 16-chain tiles: chain initialisation, the HMC transition and the step-size rule kernels that follow it
// (point creation and the Metropolis transition: ais_tile16_metropolis.hip).
//
// One workgroup (256 threads, one wave per SIMD) owns 16 chains for a whole transition: every
// leapfrog's flow log-density + gradient (fp32 MFMA, flow_device.h), target log-density + gradient,
// momentum/position updates, the Metropolis test, the in-place commit and the AIS log-weight
// increment happen inside ONE launch; the only cross-workgroup quantity (mean acceptance, needed
// for the shared `common_epsilon`) is reduced by a one-wave follow-up kernel from per-block partials
// in a fixed order (deterministic).
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
// AIS chain initialisation (ais.py:55-64): x, log_q0 = flow.sample(eps0); point = create_point(x);
// log_w = pi_beta1(point) - log_q0.   With GRAD (HMC) log q is re-evaluated through log_prob, as the
// reference does (base.py:65-68 ignores the supplied log_q_x).
// ------------------------------------------------------------------------------------------------
// MIX (defensive mixture, defensive_device.h): the whole tile runs the flow's sampler, then row i keeps the flow's x iff
// sel[i] < sigmoid(logit) and takes loc + exp(log_scale) eps0[i] otherwise; log q0 is the mixture density at x from the density
// direction (the reference's sample_and_log_prob is log_prob(sample())), so the density pass runs for Metropolis too.
template <int NTWM, bool GRAD, bool FAST, bool MIX = false>
__device__ __forceinline__ void ais_init_body(const FlowDims& f, const FlowLds& l, const ExtraLds& x,
                                              const float* __restrict__ packed, const TargetDev& tg,
                                              const float* __restrict__ eps0, const PointDev& pt, float* __restrict__ log_w,
                                              float* __restrict__ base_log_w, const fabhip_anneal& an, long B, float* lds,
                                              const MixDev& mx = MixDev{}, const float* __restrict__ sel = nullptr) {
    Tid t;
    const int D = f.D;
    const long row0 = (long)blockIdx.x * ROWS;
    float* XP = lds + x.o_XP;
    float* GP = lds + x.o_GP;
    float* MP = lds + x.total;
    if constexpr (MIX) mix_stage(mx, D, MP, t);
    zero_dp(l, lds, t);
    for (int e = t.tid; e < ROWS * l.DS; e += NTHREADS) {
        const int r = e / l.DS, j = e % l.DS;
        const long g = row0 + r;
        lds[l.o_U0 + e] = (j < D && g < B) ? eps0[g * D + j] : 0.f;
    }
    __syncthreads();
    int xoff = 0;
    float lq0 = flow_sample_tile<NTWM>(f, l, packed, lds, t, &xoff);
    if constexpr (MIX) {
        const long gr = row0 + t.row;
        const bool from_flow = gr < B ? sel[gr] < MP[4 * D + 2] : true;
        for (int j = t.c; j < D; j += 16)
            XP[t.row * D + j] = from_flow ? lds[xoff + t.row * l.DS + j] : MP[j] + expf(MP[D + j]) * eps0[gr * D + j];
    } else {
        for (int j = t.c; j < D; j += 16) XP[t.row * D + j] = lds[xoff + t.row * l.DS + j];
    }
    __syncthreads();
    float lq = lq0;
    int goff = 0;
    if (GRAD || MIX) {
        load_state_to_u0(l, D, lds, XP, t);
        __syncthreads();
        lq = flow_log_prob_tile<NTWM, GRAD, false, FAST>(f, l, packed, lds, t, &goff);
        if constexpr (MIX) {
            lq = mix_tile<GRAD>(MP, D, XP, D, lds + goff, l.DS, lq, t);
            lq0 = lq;
        }
    }
    const float lp = target_tile<GRAD>(tg, XP, D, GP, D, t);
    const long g = row0 + t.row;
    if (g < B) {
        for (int j = t.c; j < D; j += 16) {
            pt.x[g * D + j] = XP[t.row * D + j];
            if (GRAD) {
                pt.gq[g * D + j] = lds[goff + t.row * l.DS + j];
                pt.gp[g * D + j] = GP[t.row * D + j];
            }
        }
        if (t.c == 0) {
            pt.lq[g] = lq;
            pt.lp[g] = lp;
            log_w[g] = (an.c_q * lq + an.c_p * lp) - lq0;
            if (base_log_w) base_log_w[g] = lp - lq0;          // ais.py:160 (log q of the sampling pass)
        }
    }
}

template <int NTWM, bool GRAD>
__global__ __launch_bounds__(NTHREADS) void k_ais_init(FlowDims f, FlowLds l, ExtraLds x, const float* __restrict__ packed,
                                                       TargetDev tg, const float* __restrict__ eps0, PointDev pt,
                                                       float* __restrict__ log_w, float* __restrict__ base_log_w,
                                                       fabhip_anneal an, long B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    ais_init_body<NTWM, GRAD, false>(f, l, x, packed, tg, eps0, pt, log_w, base_log_w, an, B, lds);
}
template <int NTWM, bool GRAD>
__global__ __launch_bounds__(NTHREADS) void k_ais_init_mix(FlowDims f, FlowLds l, ExtraLds x, const float* __restrict__ packed,
                                                           TargetDev tg, const float* __restrict__ eps0, PointDev pt,
                                                           float* __restrict__ log_w, float* __restrict__ base_log_w,
                                                           fabhip_anneal an, long B, MixDev mx, const float* __restrict__ sel) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    ais_init_body<NTWM, GRAD, false, true>(f, l, x, packed, tg, eps0, pt, log_w, base_log_w, an, B, lds, mx, sel);
}
// fast mode: the sampling pass stays fp32; the density the transitions continue from is the bf16-GEMM one
template <int NTWM>
__global__ __launch_bounds__(NTHREADS) void k_ais_init_fast(FlowDims f, FlowLds l, ExtraLds x,
                                                            const float* __restrict__ packed, TargetDev tg,
                                                            const float* __restrict__ eps0, PointDev pt,
                                                            float* __restrict__ log_w, float* __restrict__ base_log_w,
                                                            fabhip_anneal an, long B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    ais_init_body<NTWM, true, true>(f, l, x, packed, tg, eps0, pt, log_w, base_log_w, an, B, lds);
}

// ------------------------------------------------------------------------------------------------
// One HMC outer step (hmc.py:129-160) for 16 chains per workgroup (arguments: ais_device.h, HmcK).
// ------------------------------------------------------------------------------------------------
template <int NTWM, bool FAST, bool MIX = false>
__device__ __forceinline__ void hmc_step_body(const FlowDims& f, const FlowLds& l, const ExtraLds& x,
                                              const float* __restrict__ packed, const TargetDev& tg, const HmcK& a,
                                              float* lds, const MixDev& mx = MixDev{}) {
    Tid t;
    const int D = f.D;
    const long nv = a.n_valid ? (long)*a.n_valid : a.B;
    const long row0 = (long)blockIdx.x * ROWS;
    if (row0 >= nv) {
        if (t.tid == 0) { a.part_acc[blockIdx.x] = 0.f; a.part_dist[blockIdx.x] = 0.f; }
        return;
    }
    float* XP = lds + x.o_XP;
    float* P = lds + x.o_P;
    float* GU = lds + x.o_GU;
    float* GP = lds + x.o_GP;
    float* ROWB = lds + x.o_ROW;
    const long g = row0 + t.row;
    const bool active = g < nv;
    const float eps = *a.eps_ptr + *a.ceps_ptr;                     // get_epsilon (hmc.py:90-100)
    if constexpr (MIX) mix_stage(mx, D, lds + x.total, t);          // (read behind the barriers of the first leapfrog)
    zero_dp(l, lds, t);
    float k0 = 0.f;
    for (int j = t.c; j < D; j += 16) {
        const float m = a.mass[j];
        float xs = 0.f, p = 0.f, gu = 0.f;
        if (active) {
            xs = a.start.x[g * D + j];
            p = a.noise_p[g * D + j] * m;                           // hmc.py:134 (x mass, not sqrt)
            const float gr = -(a.c.g_q * a.start.gq[g * D + j] + a.c.g_p * a.start.gp[g * D + j]);
            gu = clamp_nan0(gr, a.max_grad);
        }
        XP[t.row * D + j] = xs; P[t.row * D + j] = p; GU[t.row * D + j] = gu;
        k0 += p * p / m;
    }
    k0 = row16_sum(k0) / 2.f;
    float lq_c = 0.f, lp_c = 0.f;
    if (active) { lq_c = a.cur.lq[g]; lp_c = a.cur.lp[g]; }
    const float logp_cur = (a.c.c_q * lq_c + a.c.c_p * lp_c) - k0;  // -U(current) - K(p0)
    float lq = 0.f, lp = 0.f;
    int goff = 0;
    for (int step = 0; step < a.L; ++step) {
        for (int j = t.c; j < D; j += 16) {
            const float m = a.mass[j];
            float p = P[t.row * D + j] - eps * GU[t.row * D + j] / 2.f;
            const float xn = XP[t.row * D + j] + eps / m * p;
            P[t.row * D + j] = p; XP[t.row * D + j] = xn;
        }
        __syncthreads();
        load_state_to_u0(l, D, lds, XP, t);
        __syncthreads();
        lq = flow_log_prob_tile<NTWM, true, false, FAST>(f, l, packed, lds, t, &goff);
        if constexpr (MIX) lq = mix_tile<true>(lds + x.total, D, XP, D, lds + goff, l.DS, lq, t);
        lp = target_tile<true>(tg, XP, D, GP, D, t);
        for (int j = t.c; j < D; j += 16) {
            const float gr = -(a.c.g_q * lds[goff + t.row * l.DS + j] + a.c.g_p * GP[t.row * D + j]);
            const float gu = clamp_nan0(gr, a.max_grad);
            GU[t.row * D + j] = gu;
            P[t.row * D + j] = P[t.row * D + j] - eps * gu / 2.f;
        }
    }
    // Metropolis test (hmc.py:105-124)
    float k1 = 0.f, dist2 = 0.f;
    for (int j = t.c; j < D; j += 16) {
        const float p = P[t.row * D + j];
        k1 += p * p / a.mass[j];
        if (active) { const float dx = a.cur.x[g * D + j] - XP[t.row * D + j]; dist2 += dx * dx; }
    }
    k1 = row16_sum(k1) / 2.f;
    dist2 = row16_sum(dist2);
    const float logp_prop = (a.c.c_q * lq + a.c.c_p * lp) - k1;
    const float delta = logp_prop - logp_cur;
    const bool valid = isfinite(delta);
    const float dd = valid ? delta : -INFINITY;
    bool accept = false;
    float contrib = 0.f, dist = 0.f;
    if (active) {
        accept = valid && (dd > -a.noise_e[g]);
        contrib = expf(fminf(dd, 0.f));
        dist = accept ? 0.f : sqrtf(dist2);      // store_info sees the already-committed point (hmc.py:154-156)
    }
    if (a.prop_out.x && active) {                 // n_outer > 1: the next outer step starts from the PROPOSAL
        for (int j = t.c; j < D; j += 16) {
            a.prop_out.x[g * D + j] = XP[t.row * D + j];
            a.prop_out.gq[g * D + j] = lds[goff + t.row * l.DS + j];
            a.prop_out.gp[g * D + j] = GP[t.row * D + j];
        }
        if (t.c == 0) { a.prop_out.lq[g] = lq; a.prop_out.lp[g] = lp; }
    }
    if (accept) {                                 // current_point[accept] = point[accept]
        for (int j = t.c; j < D; j += 16) {
            a.cur.x[g * D + j] = XP[t.row * D + j];
            a.cur.gq[g * D + j] = lds[goff + t.row * l.DS + j];
            a.cur.gp[g * D + j] = GP[t.row * D + j];
        }
        if (t.c == 0) { a.cur.lq[g] = lq; a.cur.lp[g] = lp; }
    }
    if (a.log_w && active && t.c == 0) {          // ais.py:93-100
        const float lqf = accept ? lq : lq_c, lpf = accept ? lp : lp_c;
        const float num = a.nx.c_q * lqf + a.nx.c_p * lpf;
        const float den = a.c.c_q * lqf + a.c.c_p * lpf;
        a.log_w[g] = a.log_w[g] + (num - den);
    }
    if (t.c == 0) { ROWB[t.row] = contrib; ROWB[ROWS + t.row] = dist; }
    __syncthreads();
    if (t.tid == 0) {
        float s = 0.f, d = 0.f;
        for (int r = 0; r < ROWS; ++r) { s += ROWB[r]; d += ROWB[ROWS + r]; }
        a.part_acc[blockIdx.x] = s;
        a.part_dist[blockIdx.x] = d;
    }
}

template <int NTWM>
__global__ __launch_bounds__(NTHREADS) void k_hmc_step(FlowDims f, FlowLds l, ExtraLds x, const float* __restrict__ packed,
                                                       TargetDev tg, HmcK a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    hmc_step_body<NTWM, false>(f, l, x, packed, tg, a, lds);
}
template <int NTWM>
__global__ __launch_bounds__(NTHREADS) void k_hmc_step_mix(FlowDims f, FlowLds l, ExtraLds x, const float* __restrict__ packed,
                                                           TargetDev tg, HmcK a, MixDev mx) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    hmc_step_body<NTWM, false, true>(f, l, x, packed, tg, a, lds, mx);
}
// fast mode (fabhip_set_fast_mode): the W x W GEMMs of every coupling layer on the bf16 matrix cores
template <int NTWM>
__global__ __launch_bounds__(NTHREADS) void k_hmc_step_fast(FlowDims f, FlowLds l, ExtraLds x,
                                                            const float* __restrict__ packed, TargetDev tg, HmcK a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    hmc_step_body<NTWM, true>(f, l, x, packed, tg, a, lds);
}

// `slab` != nullptr (chains sharded over ranks): publish [acc[nblk] | dist[nblk] | n] for the all-gather instead of
// adapting (k_hmc_adapt_gathered does that on every rank's slab, in rank order)
__global__ void k_hmc_adapt(float* __restrict__ part_acc, float* __restrict__ part_dist, int nblk,
                            const int* n_valid, long B, float* eps_ptr, float* ceps_ptr, float target_p_accept,
                            int tune, float* p_accept_out, float* dist_out, const float* __restrict__ row_acc,
                            const float* __restrict__ row_dist, float* __restrict__ slab) {
    if (row_acc) {
        for (int b = threadIdx.x; b < nblk; b += blockDim.x) {
            float s = 0.f, d = 0.f;
            for (int r = 0; r < ROWS; ++r) { s += row_acc[(long)b * ROWS + r]; d += row_dist[(long)b * ROWS + r]; }
            part_acc[b] = s; part_dist[b] = d;
        }
        __syncthreads();
    }
    const long nv = n_valid ? (long)*n_valid : B;
    if (slab) {
        for (int b = threadIdx.x; b < nblk; b += blockDim.x) { slab[b] = part_acc[b]; slab[nblk + b] = part_dist[b]; }
        if (threadIdx.x == 0) slab[2 * nblk] = (float)(nv > 0 ? nv : 0);      // (exact: chain counts are far below 2^24)
        return;
    }
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (nv <= 0) return;
    float s = 0.f, d = 0.f;
    for (int i = 0; i < nblk; ++i) { s += part_acc[i]; d += part_dist[i]; }
    hmc_adapt_rule(s, d, nv, eps_ptr, ceps_ptr, target_p_accept, tune, p_accept_out, dist_out);
}

// the slabs of all ranks, in rank order: the same additions, in the same order, as one device holding every chain
__global__ void k_hmc_adapt_gathered(const float* __restrict__ slabs, int n_ranks, int nblk, float* eps_ptr,
                                     float* ceps_ptr, float target_p_accept, int tune, float* p_accept_out,
                                     float* dist_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int stride = 2 * nblk + 1;
    float s = 0.f, d = 0.f;
    long nv = 0;
    for (int r = 0; r < n_ranks; ++r) {
        const float* sl = slabs + (long)r * stride;
        for (int i = 0; i < nblk; ++i) { s += sl[i]; d += sl[nblk + i]; }
        nv += (long)sl[2 * nblk];
    }
    if (nv <= 0) return;
    hmc_adapt_rule(s, d, nv, eps_ptr, ceps_ptr, target_p_accept, tune, p_accept_out, dist_out);
}

// ------------------------------------------------------------------------------------------------
// host-side launchers.  `mx.on` (defensive mixture, defensive_device.h): the *_mix instantiation, fp32 only, with the staged
// mixture parameters behind the kernel's LDS plan.
// ------------------------------------------------------------------------------------------------
template <int NTWM>
static int launch_ais_init(const FlowDims& f, const float* packed, const TargetDev& tg, const float* eps0,
                           const PointDev& pt, float* log_w, float* base_log_w, fabhip_anneal an, int with_grad, long B,
                           const MixDev& mx, const float* sel, hipStream_t st) {
    const Lds16 p = make_lds16(f, with_grad != 0, mx);
    const dim3 grid(nblk_of(B)), block(NTHREADS);
    if (mx.on && with_grad)
        return launch_lds(k_ais_init_mix<NTWM, true>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, eps0, pt, log_w, base_log_w, an, B, mx, sel);
    if (mx.on)
        return launch_lds(k_ais_init_mix<NTWM, false>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, eps0, pt, log_w, base_log_w, an, B, mx, sel);
    if (with_grad && f.fast)
        return launch_lds(k_ais_init_fast<NTWM>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, eps0, pt, log_w, base_log_w, an, B);
    if (with_grad)
        return launch_lds(k_ais_init<NTWM, true>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, eps0, pt, log_w, base_log_w, an, B);
    return launch_lds(k_ais_init<NTWM, false>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, eps0, pt, log_w, base_log_w, an, B);
}

template <int NTWM>
static int launch_hmc_step(const FlowDims& f, const float* packed, const TargetDev& tg, const HmcK& a, const MixDev& mx,
                           hipStream_t st) {
    const Lds16 p = make_lds16(f, true, mx);
    const dim3 grid(nblk_of(a.B)), block(NTHREADS);
    if (mx.on) return launch_lds(k_hmc_step_mix<NTWM>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, a, mx);
    if (f.fast) return launch_lds(k_hmc_step_fast<NTWM>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, a);
    return launch_lds(k_hmc_step<NTWM>, grid, block, p.bytes, st, f, p.l, p.x, packed, tg, a);
}

int ais_init_t16(const FlowDims& f, const float* packed, const TargetDev& tg, const float* eps0, const PointDev& pt, float* log_w,
                 float* base_log_w, fabhip_anneal an, int with_grad, long B, const MixDev& mx, const float* sel, hipStream_t st) {
    FAB_DISPATCH_NTW(f, launch_ais_init, f, packed, tg, eps0, pt, log_w, base_log_w, an, with_grad, B, mx, sel, st);
}

int hmc_step_t16(const FlowDims& f, const float* packed, const TargetDev& tg, const HmcK& a, const MixDev& mx, hipStream_t st) {
    FAB_DISPATCH_NTW(f, launch_hmc_step, f, packed, tg, a, mx, st);
}

int hmc_adapt(float* part_acc, float* part_dist, int nblk, const int* n_valid, long B, float* eps_ptr, float* ceps_ptr,
              float target_p_accept, int tune, float* p_accept_out, float* dist_out, const float* row_acc, const float* row_dist,
              float* slab, hipStream_t st) {
    hipLaunchKernelGGL(k_hmc_adapt, dim3(1), dim3(64), 0, st, part_acc, part_dist, nblk, n_valid, B, eps_ptr, ceps_ptr,
                       target_p_accept, tune, p_accept_out, dist_out, row_acc, row_dist, slab);
    return check_launch();
}

}  // namespace fab

using namespace fab;

extern "C" {

int64_t fabhip_hmc_partials_floats(int64_t B) { return B < 0 ? -1 : 2 * (int64_t)nblk_of(B) + 1; }

int fabhip_hmc_adapt_gathered(const float* gathered, int32_t n_ranks, int64_t B_rank, float* epsilon, float* common_epsilon,
                              float target_p_accept, int32_t tune, float* p_accept, float* avg_distance,
                              fabhip_stream_t stream) {
    if (!gathered || n_ranks < 1 || B_rank < 1 || !epsilon || !common_epsilon) return FABHIP_EINVAL;
    hipLaunchKernelGGL(k_hmc_adapt_gathered, dim3(1), dim3(64), 0, (hipStream_t)stream, gathered, n_ranks, nblk_of(B_rank),
                       epsilon, common_epsilon, target_p_accept, tune, p_accept, avg_distance);
    return check_launch();
}

}  // extern "C"
