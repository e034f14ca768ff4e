// The one-workgroup decisions on a batch of log-weights: the SMC decision (k_smc_decide) and the next temperature of an adaptive
// annealing schedule (k_next_beta).  Both run on the resampler's own fixed-point weights (resample_device.h).
#include "resample_device.h"
#include "resample_host.h"

#pragma clang fp contract(off)

namespace fab {

// ------------------------------------------------------------------------------------------------
// SMC mode of the fused AIS call: the decision in front of a transition (launch.h: SmcK).  A few thousand chains: ONE
// workgroup reduces, scans and searches; the point is gathered grid-wide afterwards (ais_moves.hip).  Every sum that decides
// is an integer sum (associative: the same bits for any reduction order): sum W < 2^62 in 64 bits, sum W^2 < 2^98 in 128.
// ------------------------------------------------------------------------------------------------
constexpr int SMC_THREADS = 1024;

__global__ __launch_bounds__(SMC_THREADS) void k_smc_decide(SmcK a) {
    __shared__ float sh_max[SMC_THREADS / 64];
    __shared__ unsigned long long sh_w[SMC_THREADS / 64];
    __shared__ unsigned long long sh_lo[SMC_THREADS], sh_hi[SMC_THREADS];
    __shared__ unsigned long long sh_run;
    __shared__ unsigned long long sh_S, sh_U;
    __shared__ int sh_F, sh_fire;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    long n0 = a.n_ptr ? (long)*a.n_ptr : a.B;
    n0 = n0 < 0 ? 0 : (n0 > a.B ? a.B : n0);
    // 1. the maximum finite log-weight (0 when there is none: fixed_point_weights)
    float mx = -INFINITY;
    for (long i = tid; i < a.B; i += SMC_THREADS) {
        const float v = a.log_w[i];
        if (a.lw_pre_out) a.lw_pre_out[i] = v;
        if (i < n0 && isfinite(v)) mx = fmaxf(mx, v);
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) sh_max[w] = mx;
    if (tid == 0) sh_run = 0ull;
    __syncthreads();
    mx = sh_max[0];
    for (int i = 1; i < SMC_THREADS / 64; ++i) mx = fmaxf(mx, sh_max[i]);
    const bool any_finite = mx != -INFINITY;
    if (!any_finite) mx = 0.f;
    // 2. W, the inclusive CDF (chunks of 1024 rows with a running total) and sum W^2 as a 128-bit integer
    unsigned long long acc_lo = 0ull, acc_hi = 0ull;
    for (long base = 0; base < n0; base += SMC_THREADS) {
        const long i = base + tid;
        const unsigned long long q = i < n0 ? fixed_weight(a.log_w[i], mx) : 0ull;
        const unsigned long long lo = q * q, hi = __umul64hi(q, q);
        acc_lo += lo;
        acc_hi += hi + (acc_lo < lo ? 1ull : 0ull);
        unsigned long long inc = q;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long t = shfl_up_u64(inc, off);
            if (lane >= off) inc += t;
        }
        if (lane == 63) sh_w[w] = inc;
        __syncthreads();
        unsigned long long woff = 0ull, tot = 0ull;
        for (int k = 0; k < SMC_THREADS / 64; ++k) { if (k < w) woff += sh_w[k]; tot += sh_w[k]; }
        if (i < n0) a.cdf[i] = sh_run + woff + inc;
        __syncthreads();
        if (tid == 0) sh_run += tot;
        __syncthreads();
    }
    sh_lo[tid] = acc_lo; sh_hi[tid] = acc_hi;
    __syncthreads();
    for (int s = SMC_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const unsigned long long l = sh_lo[tid] + sh_lo[tid + s];
            sh_hi[tid] += sh_hi[tid + s] + (l < sh_lo[tid] ? 1ull : 0ull);
            sh_lo[tid] = l;
        }
        __syncthreads();
    }
    // 3. the decision: one float64 expression in a fixed order (tests/smc_spec.py restates it)
    if (tid == 0) {
        const unsigned long long total = sh_run;
        const double S1 = (double)total;
        const double S2 = (double)sh_hi[0] * 18446744073709551616.0 + (double)sh_lo[0];
        const double ess = total > 0ull ? (S1 * S1) / ((double)n0 * S2) : 0.0;
        const int fire = (total > 0ull && ess < a.tau) ? 1 : 0;
        double u0 = *a.u;
        if (!(u0 >= 0.0 && u0 < 1.0)) u0 = 0.0;
        const Strata m = make_strata(total, u0, n0 > 0 ? n0 : 1);
        // (stratified: the offset word carries the seed - the 64 bits of u - and every stratum hashes its own offset from it)
        sh_S = m.S; sh_U = a.method == FABHIP_SMC_STRATIFIED ? (unsigned long long)__double_as_longlong(u0) : m.U;
        sh_F = m.F; sh_fire = fire;
        *a.flag = fire;
        // log of the mean weight: log_Z = logsumexp(log_w) - log(B) of the tail kernel is unchanged by the resampling
        *a.lw_common = fire ? (float)((double)mx + log(S1 * 1.4551915228366852e-11 / (double)n0)) : 0.f;
        if (a.resampled_out) *a.resampled_out = fire;
        if (a.ess_out) *a.ess_out = (float)ess;
    }
    __syncthreads();
    // 4. ancestors: first j with C[j] > t_k, t_k = (k S + U) >> F (oracle/numerical.py: systematic_fixed); stratified:
    //    U = U_k = hi64(ms_hash(seed, k) * S) (tests/resample_stratified_spec.py)
    const bool fire = sh_fire != 0;
    const bool strat = a.method == FABHIP_SMC_STRATIFIED;
    const unsigned long long S = sh_S, U = sh_U;
    const int F = sh_F;
    for (long k = tid; k < a.B; k += SMC_THREADS) {
        long r = k;
        if (fire && k < n0) {
            const unsigned long long Uk = strat ? __umul64hi(ms_hash(U, (unsigned long long)k), S) : U;
            const unsigned long long t = ((unsigned long long)k * S + Uk) >> F;
            long lo = 0, hi = n0;                       // first index with cdf > t
            while (lo < hi) {
                const long mid = (lo + hi) >> 1;
                if (a.cdf[mid] > t) hi = mid; else lo = mid + 1;
            }
            r = lo < n0 ? lo : n0 - 1;
        }
        a.anc[k] = (int)r;
        if (a.anc_out) a.anc_out[k] = (int)r;
    }
}

int smc_decide(const SmcK& a, hipStream_t st) {
    if (!a.log_w || !a.u || !a.cdf || !a.anc || !a.flag || !a.lw_common || a.B < 1 || a.B > 0x7fffffffL) return FABHIP_EINVAL;
    if (a.method != FABHIP_SMC_SYSTEMATIC && a.method != FABHIP_SMC_STRATIFIED) return FABHIP_EINVAL;
    hipLaunchKernelGGL(k_smc_decide, dim3(1), dim3(SMC_THREADS), 0, st, a);
    return check_launch();
}

// ------------------------------------------------------------------------------------------------
// Adaptive annealing schedule: the next temperature by ESS-decay bisection (launch.h: NextBetaK; include/fabhip.h:
// fabhip_next_beta states the definition, tests/adaptive_spec.py restates it).  One workgroup runs the 2 + K evaluations of
//     ess_of(v) = (sum W)^2 / (n0 sum W^2),   W = fixed-point weights of v[:n0]   (the integer sums of k_smc_decide)
// on candidates v_i = float32(lw_i + float32((delta s) d_i)).  An evaluation is two block reductions - the largest finite
// candidate, then (sum W, sum W^2) - each 6 wave shuffles and ONE 16-entry LDS stage; every 16-lane group adds the 16 wave
// partials itself (4 more shuffles) and every thread evaluates the float64 expression and the comparison (integer sums: the
// same bits in every thread), so the bisection's branch is uniform without a third barrier.  n0 <= NB_REG x 1024: lw and d stay in registers across the
// evaluations; above, every evaluation re-reads log_w / log_q / log_p (rows at and beyond n0 are never read).
// ------------------------------------------------------------------------------------------------
constexpr int NB_THREADS = 1024, NB_WAVES = NB_THREADS / 64, NB_REG = 8;

// float32(lw + float32((delta s) d)): one float64 product chain, one rounding to float32, one float32 add; ds < 0: lw itself
__device__ __forceinline__ float nb_cand(float lw, float d, double ds) {
    return ds < 0.0 ? lw : lw + (float)(ds * (double)d);
}

template <bool REG>
__device__ __forceinline__ double nb_ess(const NextBetaK& a, long n0, const float (&lw_r)[NB_REG], const float (&d_r)[NB_REG],
                                         double ds, float* sh_max, unsigned long long* sh_sum) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // 1. the largest finite candidate (0 when there is none: fixed_point_weights)
    float mx = -INFINITY;
    if (REG) {
#pragma unroll
        for (int k = 0; k < NB_REG; ++k) {
            const float v = nb_cand(lw_r[k], d_r[k], ds);          // (slots at and beyond n0 hold NaN)
            if (isfinite(v)) mx = fmaxf(mx, v);
        }
    } else {
        for (long i = tid; i < n0; i += NB_THREADS) {
            const float v = nb_cand(a.log_w[i], a.log_p[i] - a.log_q[i], ds);
            if (isfinite(v)) mx = fmaxf(mx, v);
        }
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) sh_max[w] = mx;
    __syncthreads();
    // (the 16 wave partials: one entry per lane of a 16-lane group and four more shuffles - a sixteenth of the LDS reads that
    //  every thread looping over the 16 entries costs, and the LDS pipe is what this kernel waits for)
    mx = sh_max[lane & (NB_WAVES - 1)];
    for (int off = NB_WAVES / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (mx == -INFINITY) mx = 0.f;
    // 2. sum W in 64 bits, sum W^2 in 128
    unsigned long long s1 = 0ull, lo = 0ull, hi = 0ull;
    auto add = [&](float v) {
        const unsigned long long q = fixed_weight(v, mx);
        const unsigned long long ql = q * q;
        s1 += q;
        lo += ql;
        hi += __umul64hi(q, q) + (lo < ql ? 1ull : 0ull);
    };
    if (REG) {
#pragma unroll
        for (int k = 0; k < NB_REG; ++k) add(nb_cand(lw_r[k], d_r[k], ds));
    } else {
        for (long i = tid; i < n0; i += NB_THREADS) add(nb_cand(a.log_w[i], a.log_p[i] - a.log_q[i], ds));
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o1 = shfl_xor_u64(s1, off), ol = shfl_xor_u64(lo, off), oh = shfl_xor_u64(hi, off);
        s1 += o1;
        lo += ol;
        hi += oh + (lo < ol ? 1ull : 0ull);
    }
    if (lane == 0) { sh_sum[3 * w] = s1; sh_sum[3 * w + 1] = lo; sh_sum[3 * w + 2] = hi; }
    __syncthreads();      // (sh_max is rewritten only behind this barrier, sh_sum only behind the next evaluation's first one)
    s1 = sh_sum[3 * (lane & (NB_WAVES - 1))]; lo = sh_sum[3 * (lane & (NB_WAVES - 1)) + 1]; hi = sh_sum[3 * (lane & (NB_WAVES - 1)) + 2];
    for (int off = NB_WAVES / 2; off > 0; off >>= 1) {
        const unsigned long long o1 = shfl_xor_u64(s1, off), ol = shfl_xor_u64(lo, off), oh = shfl_xor_u64(hi, off);
        s1 += o1;
        lo += ol;
        hi += oh + (lo < ol ? 1ull : 0ull);
    }
    // 3. the float64 expression of the SMC decision (tests/smc_spec.py: decide, step 2)
    if (s1 == 0ull) return 0.0;
    const double S1 = (double)s1;
    const double S2 = (double)hi * 18446744073709551616.0 + (double)lo;
    return (S1 * S1) / ((double)n0 * S2);
}

template <bool REG>
__global__ __launch_bounds__(NB_THREADS) void k_next_beta(NextBetaK a) {
    __shared__ float sh_max[NB_WAVES];
    __shared__ unsigned long long sh_sum[3 * NB_WAVES];
    const int tid = threadIdx.x;
    long n0 = a.n_ptr ? (long)*a.n_ptr : a.B;
    n0 = n0 < 0 ? 0 : (n0 > a.B ? a.B : n0);
    float lw_r[NB_REG], d_r[NB_REG];
#pragma unroll
    for (int k = 0; k < NB_REG; ++k) {
        const long i = (long)k * NB_THREADS + tid;
        const bool in = REG && i < n0;
        lw_r[k] = in ? a.log_w[i] : __builtin_nanf("");
        d_r[k] = in ? a.log_p[i] - a.log_q[i] : 0.f;
    }
    int evals = 1, floor_taken = 0;
    const double ess0 = nb_ess<REG>(a, n0, lw_r, d_r, -1.0, sh_max, sh_sum);
    const double thr = a.rho * ess0, room = 1.0 - a.beta;
    double beta_next = 1.0, ess_at = ess0;
    if (room > 0.0) {
        ess_at = nb_ess<REG>(a, n0, lw_r, d_r, room * a.s, sh_max, sh_sum);
        evals = 2;
        if (!(ess_at >= thr)) {
            double lo = 0.0, hi = room, ess_lo = ess0, ess_hi = ess_at;
            for (int it = 0; it < a.iters; ++it) {
                const double mid = 0.5 * (lo + hi);
                const double e = nb_ess<REG>(a, n0, lw_r, d_r, mid * a.s, sh_max, sh_sum);
                if (e >= thr) { lo = mid; ess_lo = e; } else { hi = mid; ess_hi = e; }
            }
            evals += a.iters;
            floor_taken = lo > 0.0 ? 0 : 1;                 // every midpoint failed: room / 2^K, so that every step moves
            const double delta = floor_taken ? hi : lo;
            ess_at = floor_taken ? ess_hi : ess_lo;
            beta_next = fmin(a.beta + delta, 1.0);
        }
    }
    if (tid == 0) {
        a.out[0] = beta_next; a.out[1] = ess0; a.out[2] = ess_at; a.out[3] = (double)(evals + 65536 * floor_taken);
    }
}

int next_beta(const NextBetaK& a, hipStream_t st) {
    if (!a.log_w || !a.log_q || !a.log_p || !a.out || a.B < 1 || a.B > 0x7fffffffL) return FABHIP_EINVAL;
    if (!(a.beta >= 0.0 && a.beta <= 1.0) || !(a.rho > 0.0 && a.rho < 1.0) || !(a.s == a.s) || a.iters < 1 || a.iters > 60)
        return FABHIP_EINVAL;
    // (the row count lives on the device: the capacity decides - B <= 8192 covers every n0 the register variant can meet)
    if (a.B <= (long)NB_REG * NB_THREADS) hipLaunchKernelGGL(k_next_beta<true>, dim3(1), dim3(NB_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_next_beta<false>, dim3(1), dim3(NB_THREADS), 0, st, a);
    return check_launch();
}

}  // namespace fab

using namespace fab;

extern "C" {

size_t fabhip_smc_workspace_bytes(int64_t B) { return al256((size_t)(B > 0 ? B : 0) * 8) + al256((size_t)(B > 0 ? B : 0) * 4) + 512; }

int fabhip_smc_decide(const float* log_w, int64_t B, const int32_t* n_ptr, double tau, const double* u, int32_t* ancestors,
                      int32_t* resampled, float* ess, float* log_w_common, float* log_w_pre, void* workspace,
                      size_t workspace_bytes, int32_t method, fabhip_stream_t stream) {
    if (!log_w || !u || !ancestors || !resampled || !log_w_common || !workspace || B < 1) return FABHIP_EINVAL;
    if (workspace_bytes < fabhip_smc_workspace_bytes(B)) return FABHIP_ENOSPC;
    SmcK k;
    k.log_w = log_w; k.n_ptr = n_ptr; k.B = (long)B; k.tau = tau; k.u = u;
    k.cdf = (unsigned long long*)workspace; k.anc = ancestors; k.flag = resampled; k.lw_common = log_w_common;
    k.resampled_out = nullptr; k.ess_out = ess; k.anc_out = nullptr; k.lw_pre_out = log_w_pre; k.method = method;
    return smc_decide(k, (hipStream_t)stream);
}

int fabhip_next_beta(const float* log_w, const float* log_q, const float* log_p, int64_t B, const int32_t* n_ptr, double beta,
                     double alpha, int32_t p_target, double rho, int32_t iters, double* out4, fabhip_stream_t stream) {
    NextBetaK k;
    k.log_w = log_w; k.log_q = log_q; k.log_p = log_p; k.n_ptr = n_ptr; k.B = (long)B; k.beta = beta;
    k.s = p_target ? 1.0 : alpha; k.rho = rho; k.iters = iters; k.out = out4;
    return next_beta(k, (hipStream_t)stream);
}

}  // extern "C"
