// ESS / log Z reductions and the one-launch tail of a chain phase, row gather, target log-prob kernel, ABI version / sizes.
// (The resamplers: resample_scan.hip - CDF in HBM - and resample_emit.hip - no CDF; the one-workgroup weight decisions:
// weight_decisions.hip.)
#include "flow_device.h"
#include "target_device.h"
#include "resample_host.h"
#include <stdlib.h>

#pragma clang fp contract(off)

namespace fab {

// ------------------------------------------------------------------------------------------------
// ESS / log Z (fab/utils/numerical.py:18-23; ais.py:80-86), float64 accumulation
// ------------------------------------------------------------------------------------------------
struct Msum {   // running (max, sum exp(x-max), sum exp(2(x-max)))
    double m, s1, s2;
};
__device__ __forceinline__ Msum msum_id() { return Msum{-INFINITY, 0.0, 0.0}; }
__device__ __forceinline__ Msum msum_merge(const Msum& a, const Msum& b) {
    if (a.m != a.m || b.m != b.m) return Msum{NAN, NAN, NAN};
    const double m = fmax(a.m, b.m);
    if (m == -INFINITY) return Msum{m, 0.0, 0.0};
    if (m == INFINITY) return Msum{m, NAN, NAN};      // softmax of +inf is NaN, like torch
    const double ea = exp(a.m - m), eb = exp(b.m - m);
    return Msum{m, a.s1 * ea + b.s1 * eb, a.s2 * ea * ea + b.s2 * eb * eb};
}
__device__ __forceinline__ Msum msum_push(const Msum& a, double x) {
    if (x != x || a.m != a.m) return Msum{NAN, NAN, NAN};
    if (x == INFINITY) return Msum{x, NAN, NAN};        // softmax(+inf) is NaN in torch, logsumexp +inf: the maximum is kept
    if (x == -INFINITY) return a;                       // weight 0
    if (x <= a.m) {
        const double e = (double)expf((float)(x - a.m));   // fp32 exp (1e-7 rel), fp64 accumulation
        return Msum{a.m, a.s1 + e, a.s2 + e * e};
    }
    const double r = (double)expf((float)(a.m - x));    // a.m == -inf -> 0
    return Msum{x, a.s1 * r + 1.0, a.s2 * r * r + 1.0};
}

// logsumexp of what was pushed: +inf where a weight was +inf and none NaN (torch.logsumexp; the sums are NaN there)
__device__ __forceinline__ double msum_lse(const Msum& v) { return v.m == INFINITY ? v.m : v.m + log(v.s1); }

// tree over the first `bdim` threads of the workgroup (every thread of the workgroup must call it: barriers)
__device__ __forceinline__ Msum msum_block_reduce(Msum v, Msum* sh, int bdim) {
    const int tid = threadIdx.x;
    if (tid < bdim) sh[tid] = v;
    __syncthreads();
    for (int s = bdim >> 1; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = msum_merge(sh[tid], sh[tid + s]);
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ Msum msum_block_reduce(Msum v, Msum* sh) { return msum_block_reduce(v, sh, (int)blockDim.x); }

constexpr int ESS_THREADS = 256;
constexpr int ESS_MAX_BLOCKS = 1024;

// chunk of values -> (max, sum exp(x - max), sum exp(2 (x - max))) with ONE rescale per chunk: the max is taken in fp32
// first, the exponentials are fp32 (1e-7 relative) and summed in fp32 over the <= 16 values of the chunk, the running
// totals are float64.  Same special values as torch's softmax: NaN or +inf anywhere -> NaN sums, -inf -> weight 0.
template <int NV>
__device__ __forceinline__ Msum msum_push_chunk(const Msum& a, const float (&x)[NV]) {
    float m = -INFINITY;
    bool nan = false, pinf = false;
#pragma unroll
    for (int i = 0; i < NV; ++i) { nan |= x[i] != x[i]; pinf |= x[i] == INFINITY; m = fmaxf(m, x[i]); }
    if (nan || a.m != a.m) return Msum{NAN, NAN, NAN};
    if (pinf) return Msum{INFINITY, NAN, NAN};          // (as msum_push)
    if (m == -INFINITY) return a;                       // every weight of the chunk is zero
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) { const float e = expf(x[i] - m); s1 += e; s2 += e * e; }
    const double md = (double)m;
    if (md <= a.m) {
        const double r = (double)expf((float)(md - a.m));
        return Msum{a.m, a.s1 + r * (double)s1, a.s2 + r * r * (double)s2};
    }
    const double r = (double)expf((float)(a.m - md));   // a.m == -inf -> 0
    return Msum{md, a.s1 * r + (double)s1, a.s2 * r * r + (double)s2};
}

// the work of block `vb` of `nb` of the partial pass (ltid = thread in the block): shared by k_ess_partial and the one-launch
// tail kernel, which runs the blocks one after the other - the same additions in the same order, bit for bit
// (`bdim`: threads per block of the partial pass; threads beyond it - the tail kernel runs 1024 - only keep the barriers company)
__device__ __forceinline__ Msum ess_partial_body(const float* __restrict__ lw, long n, int vb, int nb, Msum* sh, int bdim) {
    Msum v = msum_id();
    const long stride = (long)nb * bdim;
    const long tid = (long)vb * bdim + threadIdx.x;
    long done = 0;
    if ((int)threadIdx.x >= bdim) return msum_block_reduce(v, sh, bdim);
    if ((((size_t)lw) & 15) == 0) {                     // 16 values per thread per step: four coalesced 16-byte loads
        const long n16 = n / (16 * stride) * (16 * stride);
        const float4* p4 = reinterpret_cast<const float4*>(lw);
        for (long base = 0; base < n16; base += 16 * stride) {
            float x[16];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float4 q = p4[(base >> 2) + h * stride + tid];
                x[4 * h] = q.x; x[4 * h + 1] = q.y; x[4 * h + 2] = q.z; x[4 * h + 3] = q.w;
            }
            v = msum_push_chunk<16>(v, x);
        }
        done = n16;
    }
    for (long i = done + tid; i < n; i += stride) v = msum_push(v, (double)lw[i]);
    return msum_block_reduce(v, sh, bdim);
}
__device__ __forceinline__ Msum ess_partial_body(const float* __restrict__ lw, long n, int vb, int nb, Msum* sh) {
    return ess_partial_body(lw, n, vb, nb, sh, (int)blockDim.x);
}
__device__ __forceinline__ void ess_final_body(const Msum* __restrict__ part, int nblk, long n, double n_norm,
                                               float* __restrict__ out, Msum* sh, int bdim) {
    Msum v = msum_id();
    if ((int)threadIdx.x < bdim)
        for (int i = threadIdx.x; i < nblk; i += bdim) v = msum_merge(v, part[i]);
    v = msum_block_reduce(v, sh, bdim);
    if (threadIdx.x == 0) {
        const double ess = (v.s1 * v.s1 / v.s2) / (double)n;       // 1 / sum(softmax^2) / n
        const double logz = msum_lse(v) - log(n_norm);             // logsumexp - log(n_norm)
        out[0] = (float)ess;
        out[1] = (float)logz;
        out[2] = (float)n;
    }
}

__global__ __launch_bounds__(ESS_THREADS) void k_ess_partial(const float* __restrict__ lw, long n_cap, const int* n_ptr,
                                                             Msum* __restrict__ part) {
    __shared__ Msum sh[ESS_THREADS];
    const long n = n_ptr ? (long)*n_ptr : n_cap;
    const Msum v = ess_partial_body(lw, n, blockIdx.x, gridDim.x, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ __launch_bounds__(ESS_THREADS) void k_ess_final(const Msum* __restrict__ part, int nblk, long n_cap,
                                                           const int* n_ptr, double n_norm, float* __restrict__ out) {
    __shared__ Msum sh[ESS_THREADS];
    const long n = n_ptr ? (long)*n_ptr : n_cap;
    ess_final_body(part, nblk, n, n_norm, out, sh, (int)blockDim.x);
}

// ------------------------------------------------------------------------------------------------
// The tail of a chain phase for SMALL batches in ONE launch (launch.h: TailArgs; <= 2048 rows): stable compaction of the
// rows with finite log_p and log_q (ais.py:190-213), optionally log_p - log_q, then ESS / log Z over the survivors - what
// k_valid_scan, k_compact_scatter, k_compact_copyback, k_sub, k_ess_partial and k_ess_final do in six launches (~5 us each on an
// otherwise idle GPU: the work of 1024 rows is a few hundred nanoseconds).  One workgroup: the rows move IN PLACE, in row order,
// through an LDS chunk (destination <= source, so a chunk's writes only touch rows already read); nothing moves when no row was
// dropped.  The ESS runs the partial pass's blocks one after the other (ess_partial_body): bit-identical to the two-kernel form.
// ------------------------------------------------------------------------------------------------
constexpr int TAIL_THREADS = 1024;                     // scan / move / difference on 1024 threads, the ESS on the first ESS_THREADS
constexpr int TAIL_CHUNK = 32;                         // rows staged in LDS per step of the in-place move
constexpr int TAIL_MAX_BLOCKS = 2;                     // ESS blocks of 1024 values: batches of <= 2048 rows (tools/time_tail.py: one
                                                       // workgroup is level with the separate kernels at 2048 rows and behind from 4096)

__global__ __launch_bounds__(TAIL_THREADS) void k_tail_small(TailArgs a, int* __restrict__ dest, int nb) {
    extern __shared__ __attribute__((aligned(16))) float stage[];          // [TAIL_CHUNK][3 D + 4]
    __shared__ Msum sh[ESS_THREADS];
    __shared__ Msum part[TAIL_MAX_BLOCKS];
    __shared__ int wsum[TAIL_THREADS / 64];
    __shared__ int running;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NWV = TAIL_THREADS / 64;
    const long n_in = a.n_in ? (long)*a.n_in : a.B;
    if (tid == 0) { running = 0; if (a.zero_word) *a.zero_word = 0; }
    if (a.zero_f && tid < a.n_zero_f) a.zero_f[tid] = 0.f;
    __syncthreads();
    for (long base = 0; base < n_in; base += TAIL_THREADS) {               // k_valid_scan's ranks (integers: any order of work agrees)
        const long r = base + tid;
        const bool v = r < n_in && isfinite(a.lq[r]) && isfinite(a.lp[r]);
        const unsigned long long bal = __ballot(v);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int i = 0; i < NWV; ++i) { if (i < w) woff += wsum[i]; tot += wsum[i]; }
        if (r < n_in) dest[r] = v ? running + woff + pre : -1;
        __syncthreads();
        if (tid == 0) running += tot;
        __syncthreads();
    }
    const long n_out = running;
    if (tid == 0) *a.n_out = (int)n_out;
    const int D = a.D, RW = 3 * D + 4;
    const bool hg = a.gq != nullptr;
    if (n_out != n_in) {
        for (long r0 = 0; r0 < n_in; r0 += TAIL_CHUNK) {
            const int nr = (int)(n_in - r0 < TAIL_CHUNK ? n_in - r0 : TAIL_CHUNK);
            for (int e = tid; e < nr * D; e += TAIL_THREADS) {
                const int i = e / D, j = e % D;
                const long r = r0 + i;
                float* o = stage + i * RW;
                o[j] = a.x[r * D + j];
                if (hg) { o[D + j] = a.gq[r * D + j]; o[2 * D + j] = a.gp[r * D + j]; }
            }
            if (tid < nr) {
                const long r = r0 + tid;
                float* o = stage + tid * RW;
                o[3 * D] = a.lq[r]; o[3 * D + 1] = a.lp[r]; o[3 * D + 2] = a.log_w[r];
                if (a.extra) o[3 * D + 3] = a.extra[r];
            }
            __syncthreads();
            for (int e = tid; e < nr * D; e += TAIL_THREADS) {
                const int i = e / D, j = e % D;
                const long d = dest[r0 + i];
                if (d < 0 || d == r0 + i) continue;
                const float* o = stage + i * RW;
                a.x[d * D + j] = o[j];
                if (hg) { a.gq[d * D + j] = o[D + j]; a.gp[d * D + j] = o[2 * D + j]; }
            }
            if (tid < nr) {
                const long d = dest[r0 + tid];
                if (d >= 0 && d != r0 + tid) {
                    const float* o = stage + tid * RW;
                    a.lq[d] = o[3 * D]; a.lp[d] = o[3 * D + 1]; a.log_w[d] = o[3 * D + 2];
                    if (a.extra) a.extra[d] = o[3 * D + 3];
                }
            }
            __syncthreads();
        }
    }
    const float* lw = a.log_w;
    if (a.diff) {
        for (long i = tid; i < a.B; i += TAIL_THREADS) a.diff[i] = a.lp[i] - a.lq[i];
        lw = a.diff;
    }
    __syncthreads();
    for (int vb = 0; vb < nb; ++vb) {
        const Msum v = ess_partial_body(lw, n_out, vb, nb, sh, ESS_THREADS);
        if (tid == 0) part[vb] = v;
        __syncthreads();
    }
    if (nb == 1) {
        // k_ess_final with one partial merges it with 255 identities: msum_merge(v, identity) == v bit for bit (exp(0) = 1,
        // exp(-inf) = 0; -inf and NaN maxima propagate the same way), so the tree is skipped
        if (tid == 0) {
            const Msum v = msum_merge(msum_id(), part[0]);
            const double ess = (v.s1 * v.s1 / v.s2) / (double)n_out;
            const double logz = msum_lse(v) - log(a.n_norm);
            a.stats_out[0] = (float)ess; a.stats_out[1] = (float)logz; a.stats_out[2] = (float)n_out;
        }
    } else {
        ess_final_body(part, nb, n_out, a.n_norm, a.stats_out, sh, ESS_THREADS);
    }
}

__global__ void k_gather_rows(const float* __restrict__ src, const long long* __restrict__ idx, float* __restrict__ dst,
                              long n_out, long row_len) {
    if ((row_len & 3) == 0 && ((size_t)src & 15) == 0 && ((size_t)dst & 15) == 0) {
        const long r4 = row_len >> 2;
        const long total = n_out * r4;
        for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
            const long k = e / r4, j = e % r4;
            reinterpret_cast<float4*>(dst)[e] = reinterpret_cast<const float4*>(src)[idx[k] * r4 + j];
        }
    } else {
        const long total = n_out * row_len;
        for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
            const long k = e / row_len, j = e % row_len;
            dst[e] = src[idx[k] * row_len + j];
        }
    }
}

// standalone target log-prob (+grad) kernel
template <bool GRAD>
__global__ __launch_bounds__(NTHREADS) void k_target(TargetDev tg, const float* __restrict__ x, float* __restrict__ lp,
                                                     float* __restrict__ grad, long B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    Tid t;
    const int D = tg.dim;
    float* X = lds;
    float* G = lds + ROWS * D;
    const long row0 = (long)blockIdx.x * ROWS;
    for (int e = t.tid; e < ROWS * D; e += NTHREADS) {
        const long g = row0 + e / D;
        X[e] = g < B ? x[g * D + e % D] : 0.f;
    }
    __syncthreads();
    const float v = target_tile<GRAD>(tg, X, D, G, D, t);
    const long g = row0 + t.row;
    if (g < B) {
        if (t.c == 0) lp[g] = v;
        if (GRAD) for (int j = t.c; j < D; j += 16) grad[g * D + j] = G[t.row * D + j];
    }
}

int tail_small(const TailArgs& a, int* dest, hipStream_t st) {
    if (a.B > (long)TAIL_MAX_BLOCKS * ESS_THREADS * 4 || a.B < 1) return FABHIP_ENOTSUP;
    const int nb = grid_for(a.B, ESS_THREADS * 4, ESS_MAX_BLOCKS);          // fabhip_ess_logz's grid for the same row capacity
    const size_t bytes = (size_t)TAIL_CHUNK * (3 * a.D + 4) * 4;
    if (bytes > 48 * 1024) return FABHIP_ENOTSUP;
    hipLaunchKernelGGL(k_tail_small, dim3(1), dim3(TAIL_THREADS), bytes, st, a, dest, nb);
    return check_launch();
}

}  // namespace fab

using namespace fab;

extern "C" {

const char* fabhip_strerror(int code) {
    switch (code) {
        case FABHIP_OK: return "ok";
        case FABHIP_EINVAL: return "invalid argument (shape, null pointer or alignment)";
        case FABHIP_ENOTSUP: return "not supported (dimension beyond compiled limits)";
        case FABHIP_ELAUNCH: return "kernel launch failed (hipGetLastError)";
        case FABHIP_ENOSPC: return "workspace too small";
        default: return "unknown fabhip error";
    }
}

int fabhip_version(void) { return FABHIP_ABI_VERSION; }

void fabhip_abi_sizes(int64_t out8[8]) {
    if (!out8) return;
    out8[0] = (int64_t)sizeof(fabhip_flow_params); out8[1] = (int64_t)sizeof(fabhip_flow);
    out8[2] = (int64_t)sizeof(fabhip_target);      out8[3] = (int64_t)sizeof(fabhip_point);
    out8[4] = (int64_t)sizeof(fabhip_anneal);      out8[5] = (int64_t)sizeof(fabhip_hmc_args);
    out8[6] = (int64_t)sizeof(fabhip_metropolis_args); out8[7] = (int64_t)sizeof(fabhip_ais_args);
}

int fabhip_target_log_prob(const fabhip_target* target, const float* x, float* log_p, float* grad_x, int64_t B,
                           fabhip_stream_t stream) {
    if (!target || !x || !log_p || B < 0) return FABHIP_EINVAL;
    if (target->dim < 1 || target->dim > FABHIP_MAX_DIM) return FABHIP_ENOTSUP;
    FAB_TRY(check_target(target, target->dim));
    if (B == 0) return FABHIP_OK;
    const TargetDev tg = make_target_dev(*target);
    const size_t bytes = (size_t)2 * ROWS * tg.dim * 4;
    const dim3 grid((unsigned)((B + ROWS - 1) / ROWS)), block(NTHREADS);
    if (grad_x) hipLaunchKernelGGL((k_target<true>), grid, block, bytes, (hipStream_t)stream, tg, x, log_p, grad_x, (long)B);
    else hipLaunchKernelGGL((k_target<false>), grid, block, bytes, (hipStream_t)stream, tg, x, log_p, grad_x, (long)B);
    return check_launch();
}

size_t fabhip_ess_workspace_bytes(int64_t n) { (void)n; return al256(sizeof(Msum) * ESS_MAX_BLOCKS) + 256; }

int fabhip_ess_logz(const float* log_w, int64_t n, const int32_t* n_ptr, double n_norm, float* out, void* workspace,
                    size_t workspace_bytes, fabhip_stream_t stream) {
    if (!log_w || !out || !workspace || n < 0) return FABHIP_EINVAL;
    if (workspace_bytes < fabhip_ess_workspace_bytes(n)) return FABHIP_ENOSPC;
    Msum* part = (Msum*)workspace;
    const int nblk = grid_for(n, ESS_THREADS * 4, ESS_MAX_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ess_partial, dim3(nblk), dim3(ESS_THREADS), 0, st, log_w, (long)n, n_ptr, part);
    hipLaunchKernelGGL(k_ess_final, dim3(1), dim3(ESS_THREADS), 0, st, part, nblk, (long)n, n_ptr, n_norm, out);
    return check_launch();
}

int fabhip_gather_rows(const float* src, const int64_t* idx, float* dst, int64_t n_out, int64_t row_len,
                       fabhip_stream_t stream) {
    if (!src || !idx || !dst || n_out < 0 || row_len < 1) return FABHIP_EINVAL;
    if (n_out == 0) return FABHIP_OK;
    hipLaunchKernelGGL(k_gather_rows, dim3(grid_for(n_out * row_len, 256 * 4, 8192)), dim3(256), 0, (hipStream_t)stream,
                       src, (const long long*)idx, dst, (long)n_out, (long)row_len);
    return check_launch();
}

}  // extern "C"
