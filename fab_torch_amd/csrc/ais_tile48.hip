// AIS inner loop on 4-chain tiles (flow_r4.h, flow_r4f.h) and on 8-chain tiles (flow_r8.h): the HMC outer step and the chain
// initialisation of each.  The two families share ONE unit on purpose: hipcc schedules k_hmc_step_r8 differently (other SGPR
// spills, another instruction order around the in-kernel step-size rule) in a module that lacks the 4-chain kernels, and the
// hand-counted waits of both families are checked on the code this unit gives.
#include "flow_device.h"
#include "target_device.h"
#include "flow_r4.h"
#include "flow_r4f.h"
#include "flow_r8.h"
#include "launch.h"

#pragma clang fp contract(off)   // keep a*b+c un-fused in the elementwise code, like the eager CPU reference

#include "ais_device.h"
#include "ais_host.h"

namespace fab {

// ------------------------------------------------------------------------------------------------
// The HMC outer step of ais_tile16.hip for FOUR chains per workgroup (flow_r4.h): used when 16-chain tiles would leave most of
// the chip idle (B <= 1152: 1024 chains = 256 workgroups instead of 64).  Element-wise work runs on wave 0 with the
// 16-chain code's (row = tid >> 4, c = tid & 15) mapping; acceptance / distance contributions go out per chain.
// ------------------------------------------------------------------------------------------------
struct ExtraLds4 {
    int o_XP, o_P, o_GU, o_GP, total;
};
static inline ExtraLds4 make_extra_lds4(const R4Lds& l, int D) {
    ExtraLds4 e;
    int o = l.total;
    e.o_XP = o; o += R4 * D;
    e.o_P = o; o += R4 * D;
    e.o_GU = o; o += R4 * D;
    e.o_GP = o; o += R4 * D;
    e.total = (o + 3) & ~3;
    return e;
}

// MODE: 0 = per-stage weight requests (flow_log_prob_r4), 1 = one stream per wave (flow_log_prob_r4s), 2 = fused stages on
// their own stream (flow_r4f.h: flow_log_prob_r4f; the bias blocks of all layers are copied to LDS once per launch), 3 = the
// fused stages in FAST mode (bf16 W x W tiles: never the parity path), 4 = the fused stages with the last R4F_NS items of every
// W x W stage prefetched into LDS during the short stages (flow_r4f.h "stash": same arithmetic, bit-identical to MODE 2)
constexpr int R4F_NS = 3;
template <int NTWM, bool BIGD, int MODE>
__global__ __launch_bounds__(NTHREADS) void k_hmc_step_r4(FlowDims f, R4Dims rd, R4Lds l, ExtraLds4 x,
                                                          const float* __restrict__ packed, TargetDev tg, HmcK a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Tid4 t4;
    Tid t;                                           // (row, c) of the element-wise mapping; valid rows: tid < 64
    const int D = f.D;
    const long nv = a.n_valid ? (long)*a.n_valid : a.B;
    const long row0 = (long)blockIdx.x * R4;
    const bool ew = t.tid < 64;
    const long g = row0 + t.row;
    if (row0 >= nv) {
        if (ew && t.c == 0 && g < (a.B + 15) / 16 * 16) hmc_store_row_stats(a, g, 0.f, 0.f);
        if (ew) hmc_adapt_last(a, lds, t.tid, 1);
        return;
    }
    float* XP = lds + x.o_XP;
    float* P = lds + x.o_P;
    float* GU = lds + x.o_GU;
    float* GP = lds + x.o_GP;
    const bool active = ew && g < nv;
    const float eps = *a.eps_ptr + *a.ceps_ptr;
    for (int e = t.tid; e < R4 * R4_DS; e += NTHREADS) { lds[l.o_DP + e] = 0.f; lds[l.o_PRM + e] = 0.f; }
    if constexpr (MODE >= 2) r4f_load_bias(packed + f.o_r4fb, lds + l.o_BIAS, f.K * r4f_bias_stride(f.Wp), t.tid);
    float k0 = 0.f;
    if (ew) {
        for (int j = t.c; j < D; j += 16) {
            const float m = a.mass[j];
            float xs = 0.f, p = 0.f, gu = 0.f;
            if (active) {
                xs = a.start.x[g * D + j];
                p = a.noise_p[g * D + j] * m;
                const float gr = -(a.c.g_q * a.start.gq[g * D + j] + a.c.g_p * a.start.gp[g * D + j]);
                gu = clamp_nan0(gr, a.max_grad);
            }
            XP[t.row * D + j] = xs; P[t.row * D + j] = p; GU[t.row * D + j] = gu;
            k0 += p * p / m;
        }
        k0 = row16_sum(k0) / 2.f;
    }
    float lq_c = 0.f, lp_c = 0.f;
    if (active) { lq_c = a.cur.lq[g]; lp_c = a.cur.lp[g]; }
    const float logp_cur = (a.c.c_q * lq_c + a.c.c_p * lp_c) - k0;
    float lq = 0.f, lp = 0.f;
    int goff = 0;
    for (int step = 0; step < a.L; ++step) {
        if (ew) {
            for (int j = t.c; j < D; j += 16) {
                const float m = a.mass[j];
                float p = P[t.row * D + j] - eps * GU[t.row * D + j] / 2.f;
                const float xn = XP[t.row * D + j] + eps / m * p;
                P[t.row * D + j] = p; XP[t.row * D + j] = xn;
            }
        }
        __syncthreads();
        for (int e = t.tid; e < R4 * R4_DS; e += NTHREADS) {
            const int r = e / R4_DS, j = e % R4_DS;
            lds[l.o_X0 + e] = j < D ? XP[r * D + j] : 0.f;
        }
        __syncthreads();
        if constexpr (MODE == 4) lq = flow_log_prob_r4f<NTWM, false, R4F_NS>(f, l, packed, lds, t4, &goff, lds + x.total);
        else if constexpr (MODE == 3) lq = flow_log_prob_r4f<NTWM, true>(f, l, packed, lds, t4, &goff);
        else if constexpr (MODE == 2) lq = flow_log_prob_r4f<NTWM>(f, l, packed, lds, t4, &goff);
        else if constexpr (MODE == 1) lq = flow_log_prob_r4s<NTWM>(f, rd, l, packed, lds, t4, &goff);
        else lq = flow_log_prob_r4<NTWM, BIGD ? 4 : 2, BIGD ? 4 : 2, BIGD ? 4 : 2, BIGD ? 2 : 1>(f, rd, l, packed, lds, t4, &goff);
        if (ew) {
            lp = target_tile<true>(tg, XP, D, GP, D, t);
            for (int j = t.c; j < D; j += 16) {
                const float gr = -(a.c.g_q * lds[goff + t.row * R4_DS + j] + a.c.g_p * GP[t.row * D + j]);
                const float gu = clamp_nan0(gr, a.max_grad);
                GU[t.row * D + j] = gu;
                P[t.row * D + j] = P[t.row * D + j] - eps * gu / 2.f;
            }
        }
    }
    if (!ew) return;
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
        dist = accept ? 0.f : sqrtf(dist2);
    }
    // (first: the latency of the write-through stores of the in-kernel step-size rule hides behind the commit stores)
    if (t.c == 0 && g < (a.B + 15) / 16 * 16) hmc_store_row_stats(a, g, contrib, dist);
    if (a.prop_out.x && active) {
        for (int j = t.c; j < D; j += 16) {
            a.prop_out.x[g * D + j] = XP[t.row * D + j];
            a.prop_out.gq[g * D + j] = lds[goff + t.row * R4_DS + j];
            a.prop_out.gp[g * D + j] = GP[t.row * D + j];
        }
        if (t.c == 0) { a.prop_out.lq[g] = lq; a.prop_out.lp[g] = lp; }
    }
    if (accept) {
        for (int j = t.c; j < D; j += 16) {
            a.cur.x[g * D + j] = XP[t.row * D + j];
            a.cur.gq[g * D + j] = lds[goff + t.row * R4_DS + j];
            a.cur.gp[g * D + j] = GP[t.row * D + j];
        }
        if (t.c == 0) { a.cur.lq[g] = lq; a.cur.lp[g] = lp; }
    }
    if (a.log_w && active && t.c == 0) {
        const float lqf = accept ? lq : lq_c, lpf = accept ? lp : lp_c;
        const float num = a.nx.c_q * lqf + a.nx.c_p * lpf;
        const float den = a.c.c_q * lqf + a.c.c_p * lpf;
        a.log_w[g] = a.log_w[g] + (num - den);
    }
    hmc_adapt_last(a, lds, t.tid, 1);                 // (wave 0 is the only wave left)
}

// Chain initialisation on 4-chain tiles (HMC runs of <= 1152 chains): the flow SAMPLE stays on the 16-chain kernel
// (fabhip_flow_sample: no 4-chain tile code for that direction), this kernel re-evaluates log q + d/dx at the samples (the
// reference does, base.py:65-68), the target and the initial log-weight - two of the three flow passes of k_ais_init on
// 256 instead of 64 workgroups.
template <int NTWM, int MODE>
__global__ __launch_bounds__(NTHREADS) void k_ais_init_r4(FlowDims f, R4Dims rd, R4Lds l, ExtraLds4 x,
                                                          const float* __restrict__ packed, TargetDev tg,
                                                          const float* __restrict__ lq0, const float* __restrict__ eps0,
                                                          PointDev pt, float* __restrict__ log_w,
                                                          float* __restrict__ base_log_w, fabhip_anneal an, long B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Tid4 t4;
    Tid t;
    const int D = f.D;
    const long row0 = (long)blockIdx.x * R4;
    const bool ew = t.tid < 64;
    const long g = row0 + t.row;
    float* XP = lds + x.o_XP;
    float* GP = lds + x.o_GP;
    float q0s = 0.f;                                   // log q of the sampling pass (eps0 given: the flow SAMPLE runs here as well)
    bool sampled = false;
    if constexpr (MODE >= 1) {
        if (eps0) {                                    // x, log q0 = flow.sample(eps0) on this tile (k_flow_sample_r4's work)
            for (int e = t.tid; e < R4 * R4_DS; e += NTHREADS) {
                const int r = e / R4_DS, j = e % R4_DS;
                lds[l.o_X0 + e] = (j < D && row0 + r < B) ? eps0[(row0 + r) * D + j] : 0.f;
            }
            if constexpr (MODE >= 2)                   // the sampling direction's bias blocks (K + 1 virtual layers)
                r4f_load_bias(packed + f.o_r4fb + (size_t)f.K * r4f_bias_stride(f.Wp), lds + l.o_BIAS,
                              (f.K + 1) * r4f_bias_stride(f.Wp), t.tid);
            __syncthreads();
            int xoff = 0;
            if constexpr (MODE >= 2) q0s = flow_sample_r4f<NTWM>(f, l, packed, lds, t4, &xoff);       // (the sample stays fp32)
            else q0s = flow_sample_r4s<NTWM>(f, rd, l, packed, lds, t4, &xoff);
            for (int e = t.tid; e < R4 * D; e += NTHREADS) {
                const int r = e / D, j = e % D;
                const float v = lds[xoff + r * R4_DS + j];
                XP[r * D + j] = v;
                if (row0 + r < B) pt.x[(row0 + r) * D + j] = v;
            }
            __syncthreads();
            sampled = true;
        }
    }
    for (int e = t.tid; e < R4 * R4_DS; e += NTHREADS) { lds[l.o_DP + e] = 0.f; lds[l.o_PRM + e] = 0.f; }
    for (int e = t.tid; e < R4 * R4_DS; e += NTHREADS) {
        const int r = e / R4_DS, j = e % R4_DS;
        float v;
        if (sampled) v = (j < D && row0 + r < B) ? XP[r * D + j] : 0.f;
        else v = (j < D && row0 + r < B) ? pt.x[(row0 + r) * D + j] : 0.f;
        lds[l.o_X0 + e] = v;
        if (j < D) XP[r * D + j] = v;
    }
    if constexpr (MODE >= 2) r4f_load_bias(packed + f.o_r4fb, lds + l.o_BIAS, f.K * r4f_bias_stride(f.Wp), t.tid);
    __syncthreads();
    int goff = 0;
    float lq;
    if constexpr (MODE == 3) lq = flow_log_prob_r4f<NTWM, true>(f, l, packed, lds, t4, &goff);
    else if constexpr (MODE == 2) lq = flow_log_prob_r4f<NTWM>(f, l, packed, lds, t4, &goff);
    else if constexpr (MODE == 1) lq = flow_log_prob_r4s<NTWM>(f, rd, l, packed, lds, t4, &goff);
    else lq = flow_log_prob_r4<NTWM, 2, 2, 2, 1>(f, rd, l, packed, lds, t4, &goff);
    if (!ew) return;
    const float lp = target_tile<true>(tg, XP, D, GP, D, t);
    if (g < B) {
        for (int j = t.c; j < D; j += 16) {
            pt.gq[g * D + j] = lds[goff + t.row * R4_DS + j];
            pt.gp[g * D + j] = GP[t.row * D + j];
        }
        if (t.c == 0) {
            const float q0 = sampled ? q0s : lq0[g];
            pt.lq[g] = lq;
            pt.lp[g] = lp;
            log_w[g] = (an.c_q * lq + an.c_p * lp) - q0;
            if (base_log_w) base_log_w[g] = lp - q0;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------------
// 4-chain tiles pay when 16-chain tiles cannot fill the chip: up to 288 workgroups of 4 chains (B <= 1152); off in fast
// mode (no bf16 variant of the 4-chain kernel).  FABHIP_OPT_TILE_SHAPE = 16 / 4 forces the choice (tests exercise both).
// Shapes: D <= 32 and hidden width <= 320 only - the D > 32 and the 512-wide instantiations of the 4-chain kernel spill
// registers (hipcc: 52 .. 772 VGPRs), so they are neither compiled nor selectable (16-chain tiles there).
// (use_r4_tiles: launch.h - the flow sample follows the same choice)
long long* debug_timeline(hipStream_t st);           // flow_kernels.hip (dev-only stage stamps)

// The MODE ladder stands twice, in the step and in the init launcher: the step has a MODE the init kernel lacks (4, the stash) and
// takes the stream image on another condition, and every branch clamps NS for itself so that no kernel is instantiated that
// use_r4_tiles could never select - one shared ladder would need a flag per difference.
template <int NTWM>
static int launch_hmc_step_r4(const FlowDims& f0, const float* packed, const TargetDev& tg, const HmcK& a, hipStream_t st) {
    FlowDims f = f0;
    f.timeline = debug_timeline(st);
    const R4Dims rd = make_r4_dims(f);
    const bool fused = use_r4_fused(f);
    const R4Lds l = make_r4_lds(f, fused);
    const ExtraLds4 x = make_extra_lds4(l, f.D);
    const size_t bytes = (size_t)x.total * 4;
    // every row of the ceil(B / 16) sixteen-row blocks k_hmc_adapt sums is written by some workgroup (workgroups past
    // the last chain take the early-return branch and write zeros): the scratch is never read uninitialised
    const dim3 grid((unsigned)(nblk_of(a.B) * (ROWS / R4))), block(NTHREADS);
    const bool stream = option(FABHIP_OPT_R4_STREAM) != 0;  // 0: per-stage request groups also where the stream image exists
    if constexpr (NTWM > 5) {
        return FABHIP_ENOTSUP;                              // (use_r4_tiles never selects it)
    } else if (NTWM >= 2 && fused && f.fast) {
        constexpr int NS = NTWM >= 2 ? NTWM : 2;
        return launch_lds(k_hmc_step_r4<NS, false, 3>, grid, block, bytes, st, f, rd, l, x, packed, tg, a);
    } else if (NTWM >= 4 && fused && option(FABHIP_OPT_R4_STREAM) >= 3 && bytes + (size_t)R4F_NS * NTWM * NWAVE * 1024 <= 160 * 1024) {
        constexpr int NS = NTWM >= 4 ? NTWM : 4;           // (the stash exists where a layer has no empty ring items: 4 / 5 tiles per wave)
        const size_t bytes_s = bytes + (size_t)R4F_NS * NS * NWAVE * 1024;
        return launch_lds(k_hmc_step_r4<NS, false, 4>, grid, block, bytes_s, st, f, rd, l, x, packed, tg, a);
    } else if (NTWM >= 2 && fused) {
        constexpr int NS = NTWM >= 2 ? NTWM : 2;
        return launch_lds(k_hmc_step_r4<NS, false, 2>, grid, block, bytes, st, f, rd, l, x, packed, tg, a);
    } else if (NTWM >= 2 && f.o_r4s >= 0 && (stream || NTWM >= 5)) {    // (the per-stage schedule spills at 5 tiles per wave)
        constexpr int NS = NTWM >= 2 ? NTWM : 2;           // (never instantiates the stream code for NTWM = 1)
        return launch_lds(k_hmc_step_r4<NS, false, 1>, grid, block, bytes, st, f, rd, l, x, packed, tg, a);
    } else if constexpr (NTWM < 5) {
        return launch_lds(k_hmc_step_r4<NTWM, false, 0>, grid, block, bytes, st, f, rd, l, x, packed, tg, a);
    } else {
        return FABHIP_ENOTSUP;
    }
}

template <int NTWM>
static int launch_ais_init_r4(const FlowDims& f, const float* packed, const TargetDev& tg, const float* lq0, const float* eps0,
                              const PointDev& pt, float* log_w, float* base_log_w, fabhip_anneal an, long B, hipStream_t st) {
    const R4Dims rd = make_r4_dims(f);
    const bool fused = use_r4_fused(f);
    const R4Lds l = make_r4_lds(f, fused);
    const ExtraLds4 x = make_extra_lds4(l, f.D);
    const size_t bytes = (size_t)x.total * 4;
    const dim3 grid((unsigned)((B + R4 - 1) / R4)), block(NTHREADS);
    if constexpr (NTWM > 5) {
        return FABHIP_ENOTSUP;
    } else if (NTWM >= 2 && fused && f.fast) {
        constexpr int NS = NTWM >= 2 ? NTWM : 2;
        return launch_lds(k_ais_init_r4<NS, 3>, grid, block, bytes, st, f, rd, l, x, packed, tg, lq0, eps0, pt, log_w, base_log_w, an, B);
    } else if (NTWM >= 2 && fused) {
        constexpr int NS = NTWM >= 2 ? NTWM : 2;
        return launch_lds(k_ais_init_r4<NS, 2>, grid, block, bytes, st, f, rd, l, x, packed, tg, lq0, eps0, pt, log_w, base_log_w, an, B);
    } else if (NTWM >= 2 && f.o_r4s >= 0) {
        constexpr int NS = NTWM >= 2 ? NTWM : 2;
        return launch_lds(k_ais_init_r4<NS, 1>, grid, block, bytes, st, f, rd, l, x, packed, tg, lq0, eps0, pt, log_w, base_log_w, an, B);
    } else if constexpr (NTWM < 5) {
        FAB_TRY(set_max_lds((const void*)k_ais_init_r4<NTWM, 0>, bytes));
        if (eps0) return FABHIP_ENOTSUP;                    // (the sampling direction exists on the stream image only)
        hipLaunchKernelGGL((k_ais_init_r4<NTWM, 0>), grid, block, bytes, st, f, rd, l, x, packed, tg, lq0,
                           (const float*)nullptr, pt, log_w, base_log_w, an, B);
        return check_launch();
    } else {
        return FABHIP_ENOTSUP;
    }
}

int hmc_step_r4(const FlowDims& f, const float* packed, const TargetDev& tg, const HmcK& a, hipStream_t st) {
    FAB_DISPATCH_NTW(f, launch_hmc_step_r4, f, packed, tg, a, st);
}

int ais_init_r4(const FlowDims& f, const float* packed, const TargetDev& tg, const float* lq0, const float* eps0,
                const PointDev& pt, float* log_w, float* base_log_w, fabhip_anneal an, long B, hipStream_t st) {
    FAB_DISPATCH_NTW(f, launch_ais_init_r4, f, packed, tg, lq0, eps0, pt, log_w, base_log_w, an, B, st);
}

// ------------------------------------------------------------------------------------------------
// The HMC outer step of ais_tile16.hip for EIGHT chains per workgroup (flow_r8.h; G = hidden width / 64 = 4 or 5): half the
// weight bytes per chain of the 4-chain kernel.  Element-wise work on threads < 128 with the 16-chain code's (row = tid >> 4,
// c = tid & 15) mapping; acceptance / distance contributions go out per chain, as from the 4-chain kernel.
// ------------------------------------------------------------------------------------------------
struct ExtraLds8 {
    int o_XP, o_P, o_GU, o_GP, total;
};
static inline ExtraLds8 make_extra_lds8(const R8Lds& l, int D) {
    ExtraLds8 e;
    int o = l.total;
    e.o_XP = o; o += R8 * D;
    e.o_P = o; o += R8 * D;
    e.o_GU = o; o += R8 * D;
    e.o_GP = o; o += R8 * D;
    e.total = (o + 3) & ~3;
    return e;
}

template <int G, bool FUSED>
__global__ __launch_bounds__(NTHREADS) void k_hmc_step_r8(FlowDims f, R8Lds l, ExtraLds8 x, const float* __restrict__ packed,
                                                        TargetDev tg, HmcK a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NT = NTHREADS;
    Tid8f t8;
    Tid t;                                           // (row, c) of the element-wise mapping; valid rows: tid < 128
    const int D = f.D;
    const long nv = a.n_valid ? (long)*a.n_valid : a.B;
    const long row0 = (long)blockIdx.x * R8;
    const bool ew = t.tid < 16 * R8;
    const long g = row0 + t.row;
    if (row0 >= nv) {
        if (ew && t.c == 0 && g < (a.B + 15) / 16 * 16) hmc_store_row_stats(a, g, 0.f, 0.f);
        if (ew) hmc_adapt_last(a, lds, t.tid & 63, 16 * R8 / 64);
        return;
    }
    float* XP = lds + x.o_XP;
    float* P = lds + x.o_P;
    float* GU = lds + x.o_GU;
    float* GP = lds + x.o_GP;
    const bool active = ew && g < nv;
    const float eps = *a.eps_ptr + *a.ceps_ptr;
    if constexpr (FUSED) r8f_load_heads(f, l, packed, lds, t.tid, NT);
    else r8_load_heads(f, l, packed, lds, t.tid, NT);
    for (int e = t.tid; e < R8 * R4_DS; e += NT) { lds[l.o_DP + e] = 0.f; lds[l.o_PRM + e] = 0.f; }
    std::conditional_t<FUSED, R8FStream, R8Stream> s;
    s8_stream_init(s, t8.lane);
    float k0 = 0.f;
    if (ew) {
        for (int j = t.c; j < D; j += 16) {
            const float m = a.mass[j];
            float xs = 0.f, p = 0.f, gu = 0.f;
            if (active) {
                xs = a.start.x[g * D + j];
                p = a.noise_p[g * D + j] * m;
                const float gr = -(a.c.g_q * a.start.gq[g * D + j] + a.c.g_p * a.start.gp[g * D + j]);
                gu = clamp_nan0(gr, a.max_grad);
            }
            XP[t.row * D + j] = xs; P[t.row * D + j] = p; GU[t.row * D + j] = gu;
            k0 += p * p / m;
        }
        k0 = row16_sum(k0) / 2.f;
    }
    float lq_c = 0.f, lp_c = 0.f;
    if (active) { lq_c = a.cur.lq[g]; lp_c = a.cur.lp[g]; }
    const float logp_cur = (a.c.c_q * lq_c + a.c.c_p * lp_c) - k0;
    float lq = 0.f, lp = 0.f;
    int goff = 0;
    for (int step = 0; step < a.L; ++step) {
        if (ew) {
            for (int j = t.c; j < D; j += 16) {
                const float m = a.mass[j];
                float p = P[t.row * D + j] - eps * GU[t.row * D + j] / 2.f;
                const float xn = XP[t.row * D + j] + eps / m * p;
                P[t.row * D + j] = p; XP[t.row * D + j] = xn;
            }
        }
        __syncthreads();
        for (int e = t.tid; e < R8 * R4_DS; e += NT) {
            const int r = e / R4_DS, j = e % R4_DS;
            lds[l.o_X0 + e] = j < D ? XP[r * D + j] : 0.f;
        }
        __syncthreads();
        lq = flow_log_prob_r8<G, FUSED>(f, l, packed, lds, t8, s, &goff);
        if (ew) {
            lp = target_tile<true>(tg, XP, D, GP, D, t);
            for (int j = t.c; j < D; j += 16) {
                const float gr = -(a.c.g_q * lds[goff + t.row * R4_DS + j] + a.c.g_p * GP[t.row * D + j]);
                const float gu = clamp_nan0(gr, a.max_grad);
                GU[t.row * D + j] = gu;
                P[t.row * D + j] = P[t.row * D + j] - eps * gu / 2.f;
            }
        }
    }
    if (!ew) return;
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
        dist = accept ? 0.f : sqrtf(dist2);
    }
    // (first: the latency of the write-through stores of the in-kernel step-size rule hides behind the commit stores)
    if (t.c == 0 && g < (a.B + 15) / 16 * 16) hmc_store_row_stats(a, g, contrib, dist);
    if (a.prop_out.x && active) {
        for (int j = t.c; j < D; j += 16) {
            a.prop_out.x[g * D + j] = XP[t.row * D + j];
            a.prop_out.gq[g * D + j] = lds[goff + t.row * R4_DS + j];
            a.prop_out.gp[g * D + j] = GP[t.row * D + j];
        }
        if (t.c == 0) { a.prop_out.lq[g] = lq; a.prop_out.lp[g] = lp; }
    }
    if (accept) {
        for (int j = t.c; j < D; j += 16) {
            a.cur.x[g * D + j] = XP[t.row * D + j];
            a.cur.gq[g * D + j] = lds[goff + t.row * R4_DS + j];
            a.cur.gp[g * D + j] = GP[t.row * D + j];
        }
        if (t.c == 0) { a.cur.lq[g] = lq; a.cur.lp[g] = lp; }
    }
    if (a.log_w && active && t.c == 0) {
        const float lqf = accept ? lq : lq_c, lpf = accept ? lp : lp_c;
        const float num = a.nx.c_q * lqf + a.nx.c_p * lpf;
        const float den = a.c.c_q * lqf + a.c.c_p * lpf;
        a.log_w[g] = a.log_w[g] + (num - den);
    }
    hmc_adapt_last(a, lds, t.tid & 63, 16 * R8 / 64);   // (the two element-wise waves; the others have returned)
}

// Chain initialisation on 8-chain tiles (as k_ais_init_r4: the flow SAMPLE stays on the 16-chain kernel)
template <int G, bool FUSED>
__global__ __launch_bounds__(NTHREADS) void k_ais_init_r8(FlowDims f, R8Lds l, ExtraLds8 x, const float* __restrict__ packed,
                                                        TargetDev tg, const float* __restrict__ lq0, PointDev pt,
                                                        float* __restrict__ log_w, float* __restrict__ base_log_w,
                                                        fabhip_anneal an, long B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NT = NTHREADS;
    Tid8f t8;
    Tid t;
    const int D = f.D;
    const long row0 = (long)blockIdx.x * R8;
    const bool ew = t.tid < 16 * R8;
    const long g = row0 + t.row;
    float* XP = lds + x.o_XP;
    float* GP = lds + x.o_GP;
    if constexpr (FUSED) r8f_load_heads(f, l, packed, lds, t.tid, NT);
    else r8_load_heads(f, l, packed, lds, t.tid, NT);
    for (int e = t.tid; e < R8 * R4_DS; e += NT) { lds[l.o_DP + e] = 0.f; lds[l.o_PRM + e] = 0.f; }
    for (int e = t.tid; e < R8 * R4_DS; e += NT) {
        const int r = e / R4_DS, j = e % R4_DS;
        const float v = (j < D && row0 + r < B) ? pt.x[(row0 + r) * D + j] : 0.f;
        lds[l.o_X0 + e] = v;
        if (j < D) XP[r * D + j] = v;
    }
    std::conditional_t<FUSED, R8FStream, R8Stream> s;
    s8_stream_init(s, t8.lane);
    __syncthreads();
    int goff = 0;
    const float lq = flow_log_prob_r8<G, FUSED>(f, l, packed, lds, t8, s, &goff);
    if (!ew) return;
    const float lp = target_tile<true>(tg, XP, D, GP, D, t);
    if (g < B) {
        for (int j = t.c; j < D; j += 16) {
            pt.gq[g * D + j] = lds[goff + t.row * R4_DS + j];
            pt.gp[g * D + j] = GP[t.row * D + j];
        }
        if (t.c == 0) {
            const float q0 = lq0[g];
            pt.lq[g] = lq;
            pt.lp[g] = lp;
            log_w[g] = (an.c_q * lq + an.c_p * lp) - q0;
            if (base_log_w) base_log_w[g] = lp - q0;
        }
    }
}

// 8-chain tiles (flow_r8.h: D <= 32, hidden width padded to 256 / 320, fp32): half the weight bytes per chain of the 4-chain
// kernel on one stream per wave.  FABHIP_OPT_TILE_SHAPE = 8 forces them; by default they take the batches for which
// R8_MIN_CHAINS < B <= 8 chains per CU (measured: DESIGN.md section 4).
constexpr long R8_MIN_CHAINS = 1152;
static bool r8_lds_fits(const FlowDims& f) { return (size_t)(make_r8_lds(f).total + 4 * R8 * f.D + 4) * 4 <= 160 * 1024; }
bool use_r8_tiles(const FlowDims& f, long B) {
    if (f.fast || !r8_shape_ok(f) || !r8_lds_fits(f)) return false;
    const int shape = option(FABHIP_OPT_TILE_SHAPE);
    if (shape == 16 || shape == 4) return false;
    if (shape == 8) return true;
    return B > R8_MIN_CHAINS && B <= (long)R8 * cu_count();
}

// the (G = padded width / 64, fused stages) instantiation of this flow, handed to `launch` as a tag
template <int G_, bool FUSED_>
struct R8Variant {
    static constexpr int G = G_;
    static constexpr bool FUSED = FUSED_;
};
template <class Launch>
static int dispatch_r8(const FlowDims& f, Launch&& launch) {
    const bool fused = use_r8_fused(f);
    if (f.Wp == 320) return fused ? launch(R8Variant<5, true>{}) : launch(R8Variant<5, false>{});
    if (f.Wp == 256) return fused ? launch(R8Variant<4, true>{}) : launch(R8Variant<4, false>{});
    return FABHIP_ENOTSUP;
}

int hmc_step_r8(const FlowDims& f0, const float* packed, const TargetDev& tg, const HmcK& a, hipStream_t st) {
    FlowDims f = f0;
    f.timeline = debug_timeline(st);
    const R8Lds l = make_r8_lds(f);
    const ExtraLds8 x = make_extra_lds8(l, f.D);
    const size_t bytes = (size_t)x.total * 4;
    const dim3 grid((unsigned)(nblk_of(a.B) * (ROWS / R8)));      // every row of the 16-row blocks k_hmc_adapt sums gets written
    return dispatch_r8(f, [&](auto v) {
        return launch_lds(k_hmc_step_r8<decltype(v)::G, decltype(v)::FUSED>, grid, dim3(NTHREADS), bytes, st, f, l, x, packed, tg, a);
    });
}

int ais_init_r8(const FlowDims& f, const float* packed, const TargetDev& tg, const float* lq0, const PointDev& pt, float* log_w,
                float* base_log_w, fabhip_anneal an, long B, hipStream_t st) {
    const R8Lds l = make_r8_lds(f);
    const ExtraLds8 x = make_extra_lds8(l, f.D);
    const size_t bytes = (size_t)x.total * 4;
    const dim3 grid((unsigned)((B + R8 - 1) / R8));
    return dispatch_r8(f, [&](auto v) {
        return launch_lds(k_ais_init_r8<decltype(v)::G, decltype(v)::FUSED>, grid, dim3(NTHREADS), bytes, st, f, l, x, packed, tg,
                          lq0, pt, log_w, base_log_w, an, B);
    });
}

}  // namespace fab
