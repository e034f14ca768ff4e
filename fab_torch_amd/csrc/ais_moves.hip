// Row moves of the AIS call: NaN/inf compaction, the SMC gather and copy-back, SMC over sharded chains, and the two element-wise
// kernels of the chain phases' tails.
#include "flow_device.h"
#include "launch.h"

#pragma clang fp contract(off)   // keep a*b+c un-fused in the elementwise code, like the eager CPU reference

#include "ais_device.h"
#include "ais_host.h"

namespace fab {

// ------------------------------------------------------------------------------------------------
// _remove_nan_and_infs (ais.py:190-213): stable compaction of the rows with finite log_p and log_q.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_valid_scan(const float* __restrict__ lq, const float* __restrict__ lp,
                                                     const int* n_in_ptr, long B, int* __restrict__ dest,
                                                     int* __restrict__ n_out) {
    __shared__ int wsum[16];
    __shared__ int running;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long n_in = n_in_ptr ? (long)*n_in_ptr : B;
    if (tid == 0) running = 0;
    __syncthreads();
    for (long base = 0; base < n_in; base += 1024) {
        const long r = base + tid;
        const bool v = r < n_in && isfinite(lq[r]) && isfinite(lp[r]);
        const unsigned long long bal = __ballot(v);
        const int pre = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int i = 0; i < 16; ++i) { if (i < w) woff += wsum[i]; tot += wsum[i]; }
        if (r < n_in) dest[r] = v ? running + woff + pre : -1;
        __syncthreads();
        if (tid == 0) running += tot;
        __syncthreads();
    }
    if (tid == 0) *n_out = running;
}

struct CompactK {
    PointDev pt;
    float* log_w;
    float* extra;          // optional per-row scalar carried along (nullptr: none)
    float* tmp;            // [B][3D+4]
    const int* dest;
    const int* n_in_ptr;
    const int* n_out_ptr;
    long B;
    int D;
};

__global__ void k_compact_scatter(CompactK a) {
    const long n_in = a.n_in_ptr ? (long)*a.n_in_ptr : a.B;
    const long n_out = *a.n_out_ptr;
    if (n_out == n_in) return;
    const int D = a.D, RW = 3 * D + 4;
    const bool hg = a.pt.gq != nullptr;
    for (long r = blockIdx.x; r < n_in; r += gridDim.x) {
        const int d = a.dest[r];
        if (d < 0) continue;
        float* o = a.tmp + (long)d * RW;
        for (int j = threadIdx.x; j < D; j += blockDim.x) {
            o[j] = a.pt.x[r * D + j];
            if (hg) { o[D + j] = a.pt.gq[r * D + j]; o[2 * D + j] = a.pt.gp[r * D + j]; }
        }
        if (threadIdx.x == 0) {
            o[3 * D] = a.pt.lq[r]; o[3 * D + 1] = a.pt.lp[r]; o[3 * D + 2] = a.log_w[r];
            if (a.extra) o[3 * D + 3] = a.extra[r];
        }
    }
}

__global__ void k_compact_copyback(CompactK a) {
    const long n_in = a.n_in_ptr ? (long)*a.n_in_ptr : a.B;
    const long n_out = *a.n_out_ptr;
    if (n_out == n_in) return;
    const int D = a.D, RW = 3 * D + 4;
    const bool hg = a.pt.gq != nullptr;
    for (long r = blockIdx.x; r < n_out; r += gridDim.x) {
        const float* o = a.tmp + r * RW;
        for (int j = threadIdx.x; j < D; j += blockDim.x) {
            a.pt.x[r * D + j] = o[j];
            if (hg) { a.pt.gq[r * D + j] = o[D + j]; a.pt.gp[r * D + j] = o[2 * D + j]; }
        }
        if (threadIdx.x == 0) {
            a.pt.lq[r] = o[3 * D]; a.pt.lp[r] = o[3 * D + 1]; a.log_w[r] = o[3 * D + 2];
            if (a.extra) a.extra[r] = o[3 * D + 3];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// SMC mode: the gather of the point with the ancestors of k_smc_decide (weight_decisions.hip), through the compaction's staging
// buffer and back.  Both kernels are always launched and read the device flag: the host's launch sequence is fixed.
// ------------------------------------------------------------------------------------------------
struct SmcGatherK {
    PointDev pt;
    float* log_w;
    float* tmp;            // [B][3D+4]
    const int* anc;        // [B]
    const int* flag;
    const float* lw_common;
    const int* n_ptr;
    long B;
    int D;
};

__global__ void k_smc_gather(SmcGatherK a) {
    if (*a.flag == 0) return;
    long n0 = *a.n_ptr;
    n0 = n0 < 0 ? 0 : (n0 > a.B ? a.B : n0);
    const int D = a.D, RW = 3 * D + 4;
    const bool hg = a.pt.gq != nullptr;
    for (long r = blockIdx.x; r < n0; r += gridDim.x) {
        long s = a.anc[r];
        s = s < 0 ? 0 : (s >= n0 ? n0 - 1 : s);
        float* o = a.tmp + r * RW;
        for (int j = threadIdx.x; j < D; j += blockDim.x) {
            o[j] = a.pt.x[s * D + j];
            if (hg) { o[D + j] = a.pt.gq[s * D + j]; o[2 * D + j] = a.pt.gp[s * D + j]; }
        }
        if (threadIdx.x == 0) { o[3 * D] = a.pt.lq[s]; o[3 * D + 1] = a.pt.lp[s]; }
    }
}

__global__ void k_smc_copyback(SmcGatherK a) {
    if (*a.flag == 0) return;
    long n0 = *a.n_ptr;
    n0 = n0 < 0 ? 0 : (n0 > a.B ? a.B : n0);
    const int D = a.D, RW = 3 * D + 4;
    const bool hg = a.pt.gq != nullptr;
    const float lw = *a.lw_common;
    for (long r = blockIdx.x; r < n0; r += gridDim.x) {
        const float* o = a.tmp + r * RW;
        for (int j = threadIdx.x; j < D; j += blockDim.x) {
            a.pt.x[r * D + j] = o[j];
            if (hg) { a.pt.gq[r * D + j] = o[D + j]; a.pt.gp[r * D + j] = o[2 * D + j]; }
        }
        if (threadIdx.x == 0) { a.pt.lq[r] = o[3 * D]; a.pt.lp[r] = o[3 * D + 1]; a.log_w[r] = lw; }
    }
}

// ------------------------------------------------------------------------------------------------
// SMC mode over sharded chains (include/fabhip.h: fabhip_smc_shard_pack / fabhip_smc_shard_resample).  Every rank packs its
// state into rows of RW = 3 D + 4 floats (the compaction staging's stride) + one trailer row with its live count; the host
// all-gathers the buffers; then every rank compacts the R log-weight columns into the global live order, runs k_smc_decide on
// them (the single-device kernel: its decision, ESS, ancestors and common log-weight are therefore the single-device bits)
// and fetches its own rows' ancestors out of the gathered buffer.  One wave per row; with D % 4 == 0 and 16-byte aligned
// arrays (VEC) the rows move as float4, the scalar form covers every other shape.  All kernels are always launched and read
// the device flag / counts: the launch sequence is fixed and the host never waits.
// ------------------------------------------------------------------------------------------------
constexpr int SHARD_WAVES = 4;                       // rows per workgroup
constexpr int SHARD_MAX_RANKS = 64;                  // the rank offsets are ONE wave's prefix

struct SmcShardK {
    PointDev pt;           // this rank's state [b]
    float* log_w;          // [b]
    const int* n_ptr;      // this rank's live count (device)
    float* send;           // pack: [b + 1][RW] out
    const float* gathered; // resample: [R][b + 1][RW]
    int* offs;             // workspace [R + 1]: live rows in front of rank r; offs[R] = n0
    int* n0;               // workspace [1]
    float* lw_glob;        // workspace [R b]: log_w of the live rows in global order, -inf behind them
    const int* anc;        // workspace [R b] (k_smc_decide)
    const int* flag;
    const float* lw_common;
    long b;
    int D, R, rank;
};

template <bool VEC>
__device__ inline void shard_copy(float* __restrict__ dst, const float* __restrict__ src, int n, int lane) {
    if (VEC) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int j = lane; j < n / 4; j += 64) d4[j] = s4[j];
    } else {
        for (int j = lane; j < n; j += 64) dst[j] = src[j];
    }
}

template <bool VEC>
__global__ __launch_bounds__(64 * SHARD_WAVES) void k_smc_shard_pack(SmcShardK a) {
    const int lane = threadIdx.x & 63, D = a.D, RW = 3 * D + 4;
    const bool hg = a.pt.gq != nullptr;
    const long row0 = (long)blockIdx.x * SHARD_WAVES + (threadIdx.x >> 6), stride = (long)gridDim.x * SHARD_WAVES;
    for (long r = row0; r <= a.b; r += stride) {
        float* o = a.send + r * RW;
        if (r == a.b) {                                   // the trailer: this rank's live count, bit pattern of an int32
            int n = *a.n_ptr;
            n = n < 0 ? 0 : (n > a.b ? (int)a.b : n);
            for (int j = lane; j < RW; j += 64) reinterpret_cast<int*>(o)[j] = j == 0 ? n : 0;
            continue;
        }
        shard_copy<VEC>(o, a.pt.x + r * D, D, lane);
        if (hg) {
            shard_copy<VEC>(o + D, a.pt.gq + r * D, D, lane);
            shard_copy<VEC>(o + 2 * D, a.pt.gp + r * D, D, lane);
        }
        if (lane < 4) o[3 * D + lane] = lane == 0 ? a.pt.lq[r] : (lane == 1 ? a.pt.lp[r] : (lane == 2 ? a.log_w[r] : 0.f));
    }
}

// Live counts of the R trailers -> exclusive prefix (one wave, every workgroup computes it for itself), then the log-weight
// column of every live row to its place in the global order.  Positions [n0, R b) are filled with -inf.
__global__ __launch_bounds__(256) void k_smc_shard_prefix(SmcShardK a) {
    __shared__ int sh_off[SHARD_MAX_RANKS + 1];
    const int RW = 3 * a.D + 4, R = a.R;
    if (threadIdx.x < 64) {
        const int l = threadIdx.x;
        int n = 0;
        if (l < R) {
            n = reinterpret_cast<const int*>(a.gathered)[((long)l * (a.b + 1) + a.b) * RW];
            n = n < 0 ? 0 : (n > a.b ? (int)a.b : n);
        }
        int inc = n;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(inc, off);
            if (l >= off) inc += t;
        }
        if (l < R) sh_off[l + 1] = inc;
        if (l == 0) sh_off[0] = 0;
    }
    __syncthreads();
    const long cap = (long)R * a.b;
    const int n0 = sh_off[R];
    if (blockIdx.x == 0) {
        for (int l = threadIdx.x; l <= R; l += blockDim.x) a.offs[l] = sh_off[l];
        if (threadIdx.x == 0) *a.n0 = n0;
    }
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < cap; g += (long)gridDim.x * blockDim.x) {
        const int s = (int)(g / a.b);
        const long i = g - (long)s * a.b;
        if (i < sh_off[s + 1] - sh_off[s]) a.lw_glob[sh_off[s] + i] = a.gathered[((long)s * (a.b + 1) + i) * RW + 3 * a.D + 2];
        if (g >= n0) a.lw_glob[g] = -INFINITY;
    }
}

template <bool VEC>
__global__ __launch_bounds__(64 * SHARD_WAVES) void k_smc_shard_gather(SmcShardK a) {
    if (*a.flag == 0) return;
    const int lane = threadIdx.x & 63, D = a.D, RW = 3 * D + 4, R = a.R;
    const bool hg = a.pt.gq != nullptr;
    long nr = *a.n_ptr;
    nr = nr < 0 ? 0 : (nr > a.b ? a.b : nr);
    const int n0 = a.offs[R], off_r = a.offs[a.rank];
    const int end_l = lane < R ? a.offs[lane + 1] : 0x7fffffff;       // lane s: one past the last global row of rank s
    const float lw = *a.lw_common;
    const long row0 = (long)blockIdx.x * SHARD_WAVES + (threadIdx.x >> 6), stride = (long)gridDim.x * SHARD_WAVES;
    for (long i = row0; i < nr; i += stride) {
        if (off_r + i >= n0) break;                        // (a trailer that disagrees with n_valid: nothing to fetch)
        int g = a.anc[off_r + i];
        g = g < 0 ? 0 : (g >= n0 ? n0 - 1 : g);
        // source rank = the ranks whose rows all lie in front of g (the offsets are monotone; empty ranks count themselves out)
        int s = __popcll(__ballot(end_l <= g));
        s = s > R - 1 ? R - 1 : s;
        long row = g - a.offs[s];
        row = row < 0 ? 0 : (row >= a.b ? a.b - 1 : row);
        const float* src = a.gathered + ((long)s * (a.b + 1) + row) * RW;
        shard_copy<VEC>(a.pt.x + i * D, src, D, lane);
        if (hg) {
            shard_copy<VEC>(a.pt.gq + i * D, src + D, D, lane);
            shard_copy<VEC>(a.pt.gp + i * D, src + 2 * D, D, lane);
        }
        if (lane == 0) { a.pt.lq[i] = src[3 * D]; a.pt.lp[i] = src[3 * D + 1]; a.log_w[i] = lw; }
    }
}

// ------------------------------------------------------------------------------------------------
// Flow-proposal independence move (include/fabhip.h: fabhip_flow_move; definition: tests/flow_move_spec.py): the accept /
// commit step.  `prop` is the Point of a fresh flow sample; row i takes it iff it is live, both proposal densities are finite,
// delta = r(prop) - r(cur) is a number and h_i > -delta, with r = pi_beta - log q in the expression order of
// fabhip_anneal_log_prob.  16 lanes per row: lane 0 of the group decides, the group copies the row.  The count is an integer:
// every workgroup adds (1 << 32 | its accepted rows) to ONE 64-bit word with a device-scope atomic, the workgroup that reads
// gridDim.x - 1 finished workgroups in the returned value writes the outputs and zeroes the word for the next launch.
// ------------------------------------------------------------------------------------------------
constexpr int MOVE_LANES = 16;                       // lanes per row
constexpr int MOVE_ROWS = 16;                        // rows per workgroup

struct FlowMoveK {
    PointDev cur;          // in / out
    PointDev prop;         // the proposal's Point (gq / gp null with a gradient-free operator)
    const float* h;        // [B] ~ Exp(1)
    const int* n_ptr;      // rows in use (device; null: B)
    long B;
    int D;
    fabhip_anneal c;       // beta_j
    unsigned long long* word;   // zero before the launch; zero again after it
    float* p_accept_out;   // optional [1]: n_accept / n_valid
    int* n_accept_out;     // optional [1]
};

__device__ __forceinline__ float move_ratio(const fabhip_anneal& c, float lq, float lp) { return (c.c_q * lq + c.c_p * lp) - lq; }

__global__ __launch_bounds__(MOVE_LANES * MOVE_ROWS) void k_flow_move_accept(FlowMoveK a) {
    __shared__ int wave_n[MOVE_LANES * MOVE_ROWS / 64];
    const int tid = threadIdx.x, lane = tid & 63, sub = tid & (MOVE_LANES - 1);
    long n0 = a.n_ptr ? (long)*a.n_ptr : a.B;
    n0 = n0 < 0 ? 0 : (n0 > a.B ? a.B : n0);
    const long r = (long)blockIdx.x * MOVE_ROWS + tid / MOVE_LANES;
    int acc = 0;
    if (sub == 0 && r < n0) {
        const float lqn = a.prop.lq[r], lpn = a.prop.lp[r];
        const float delta = move_ratio(a.c, lqn, lpn) - move_ratio(a.c, a.cur.lq[r], a.cur.lp[r]);
        acc = (isfinite(lqn) && isfinite(lpn) && delta == delta && a.h[r] > -delta) ? 1 : 0;
    }
    const unsigned long long bal = __ballot(acc != 0);           // (one bit per accepted row: only lane 0 of a group can set it)
    acc = __shfl(acc, lane & ~(MOVE_LANES - 1));                 // the group's decision
    if (acc) {
        const int D = a.D;
        for (int j = sub; j < D; j += MOVE_LANES) {
            a.cur.x[r * D + j] = a.prop.x[r * D + j];
            if (a.cur.gq) { a.cur.gq[r * D + j] = a.prop.gq[r * D + j]; a.cur.gp[r * D + j] = a.prop.gp[r * D + j]; }
        }
        if (sub == 0) { a.cur.lq[r] = a.prop.lq[r]; a.cur.lp[r] = a.prop.lp[r]; }
    }
    if (lane == 0) wave_n[tid >> 6] = __popcll(bal);
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int i = 0; i < MOVE_LANES * MOVE_ROWS / 64; ++i) n += wave_n[i];
        const unsigned long long old = __hip_atomic_fetch_add(a.word, (1ull << 32) | (unsigned long long)n, __ATOMIC_RELAXED,
                                                              __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)(old >> 32) == gridDim.x - 1) {            // the last workgroup: every other one's rows are in `old`
            const int total = (int)(unsigned)(old & 0xffffffffull) + n;
            if (a.n_accept_out) *a.n_accept_out = total;
            if (a.p_accept_out) *a.p_accept_out = n0 > 0 ? (float)total / (float)n0 : 0.f;
            __hip_atomic_store(a.word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ void k_sub(const float* __restrict__ a,const float* __restrict__ b, float* __restrict__ o, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) o[i] = a[i] - b[i];
}

}  // namespace fab

// ---- spline flow as base distribution (csrc/spline_stream.hip, spline_tile16.hip) ------------------------------------------------------
// (C linkage: the symbol has always been the plain name)
extern "C" __global__ void k_spline_init_logw(const float* __restrict__ lq, const float* __restrict__ lp, const float* __restrict__ lq0,
                                   fabhip_anneal an, float* __restrict__ log_w, float* __restrict__ base_log_w, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        log_w[i] = (an.c_q * lq[i] + an.c_p * lp[i]) - lq0[i];              // ais.py:62-64
        if (base_log_w) base_log_w[i] = lp[i] - lq0[i];                     // ais.py:160
    }
}

namespace fab {

// ------------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------------
int compact_rows(const fabhip_point& point, float* log_w, long B, int dim, const int* n_in, int* n_out, float* tmp, int* dest,
                 float* extra, hipStream_t st) {
    hipLaunchKernelGGL(k_valid_scan, dim3(1), dim3(1024), 0, st, point.log_q, point.log_p, n_in, B, dest, n_out);
    CompactK c{make_point_dev(point), log_w, extra, tmp, dest, n_in, n_out, B, dim};
    const int grid = (int)(B < 4096 ? B : 4096);
    hipLaunchKernelGGL(k_compact_scatter, dim3(grid), dim3(64), 0, st, c);
    hipLaunchKernelGGL(k_compact_copyback, dim3(grid), dim3(64), 0, st, c);
    return check_launch();
}

int smc_gather_copyback(const fabhip_point& point, float* log_w, float* tmp, const int* anc, const int* flag,
                        const float* lw_common, const int* n_ptr, long B, int dim, hipStream_t st) {
    SmcGatherK g{make_point_dev(point), log_w, tmp, anc, flag, lw_common, n_ptr, B, dim};
    const int grid = (int)(B < 4096 ? B : 4096);
    hipLaunchKernelGGL(k_smc_gather, dim3(grid), dim3(64), 0, st, g);
    hipLaunchKernelGGL(k_smc_copyback, dim3(grid), dim3(64), 0, st, g);
    return check_launch();
}

int flow_move_accept(const fabhip_point& cur, const PointDev& prop, const float* h, const int* n_ptr, long B, int dim,
                     fabhip_anneal c, unsigned long long* word, float* p_accept, int* n_accept, hipStream_t st) {
    FlowMoveK k{make_point_dev(cur), prop, h, n_ptr, B, dim, c, word, p_accept, n_accept};
    const long grid = (B + MOVE_ROWS - 1) / MOVE_ROWS;
    if (grid < 1 || grid > 0x7fffffffL) return FABHIP_EINVAL;
    hipLaunchKernelGGL(k_flow_move_accept, dim3((unsigned)grid), dim3(MOVE_LANES * MOVE_ROWS), 0, st, k);
    return check_launch();
}

void launch_sub(const float* a, const float* b, float* o, long n, hipStream_t st) {
    hipLaunchKernelGGL(k_sub, dim3(ceil_div((int)n, 256)), dim3(256), 0, st, a, b, o, n);
}

void launch_spline_init_logw(const float* lq, const float* lp, const float* lq0, fabhip_anneal an, float* log_w,
                             float* base_log_w, long n, hipStream_t st) {
    hipLaunchKernelGGL(k_spline_init_logw, dim3(ceil_div((int)n, 256)), dim3(256), 0, st, lq, lp, lq0, an, log_w, base_log_w, n);
}

// ---- SMC mode over sharded chains -------------------------------------------------------------------------------------------
static inline bool shard_vec_ok(const fabhip_point& p, const float* buf, int D) {
    auto al = [](const void* q) { return ((size_t)q & 15) == 0; };
    return D % 4 == 0 && al(buf) && al(p.x) && (!p.grad_log_q || (al(p.grad_log_q) && al(p.grad_log_p)));
}
static inline int shard_grid(long rows) {
    const long g = (rows + SHARD_WAVES - 1) / SHARD_WAVES;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace fab

using namespace fab;

extern "C" {

size_t fabhip_smc_shard_workspace_bytes(int32_t R, int64_t b) {
    if (R < 1 || R > SHARD_MAX_RANKS || b < 1) return 0;
    const size_t cap = (size_t)R * (size_t)b;
    // offsets [R + 1] + n0 | flag, common log-weight | global log_w | CDF | ancestors
    return 512 + 256 + al256(cap * 4) + al256(cap * 8) + al256(cap * 4);
}

int fabhip_smc_shard_pack(const fabhip_point* point, const float* log_w, const int32_t* n_valid, int64_t b, int32_t dim,
                          float* send, fabhip_stream_t stream) {
    if (!point || !point->x || !point->log_q || !point->log_p || !log_w || !n_valid || !send) return FABHIP_EINVAL;
    if ((point->grad_log_q == nullptr) != (point->grad_log_p == nullptr)) return FABHIP_EINVAL;
    if (b < 1 || b > 0x3fffffffL || dim < 1 || dim > FABHIP_MAX_DIM) return FABHIP_EINVAL;
    SmcShardK k{};
    k.pt = make_point_dev(*point); k.log_w = const_cast<float*>(log_w); k.n_ptr = n_valid; k.send = send;
    k.b = (long)b; k.D = dim; k.R = 1; k.rank = 0;
    const int grid = shard_grid((long)b + 1);
    if (shard_vec_ok(*point, send, dim)) hipLaunchKernelGGL(k_smc_shard_pack<true>, dim3(grid), dim3(64 * SHARD_WAVES), 0, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(k_smc_shard_pack<false>, dim3(grid), dim3(64 * SHARD_WAVES), 0, (hipStream_t)stream, k);
    return check_launch();
}

int fabhip_smc_shard_resample(const float* gathered, int32_t R, int32_t rank, int64_t b, int32_t dim, double tau, const double* u,
                              const fabhip_point* point, float* log_w, const int32_t* n_valid, int32_t* resampled, float* ess,
                              int32_t* ancestors, float* log_w_pre, void* workspace, size_t workspace_bytes,
                              fabhip_stream_t stream) {
    if (!gathered || !u || !point || !point->x || !point->log_q || !point->log_p || !log_w || !n_valid || !workspace)
        return FABHIP_EINVAL;
    if ((point->grad_log_q == nullptr) != (point->grad_log_p == nullptr)) return FABHIP_EINVAL;
    if (R < 1 || rank < 0 || rank >= R || b < 1 || dim < 1 || dim > FABHIP_MAX_DIM) return FABHIP_EINVAL;
    if (R > SHARD_MAX_RANKS) return FABHIP_ENOTSUP;
    if ((int64_t)R * b > 0x3fffffffL) return FABHIP_EINVAL;
    if (((size_t)workspace & 255) != 0) return FABHIP_EINVAL;
    if (workspace_bytes < fabhip_smc_shard_workspace_bytes(R, b)) return FABHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    const long cap = (long)R * (long)b;
    char* p = (char*)workspace;
    int* offs = (int*)p; int* n0 = (int*)(p + 448); p += 512;
    int* flag = (int*)p; float* common = (float*)(p + 64); p += 256;
    float* lw_glob = (float*)p; p += al256((size_t)cap * 4);
    unsigned long long* cdf = (unsigned long long*)p; p += al256((size_t)cap * 8);
    int* anc = (int*)p;
    SmcShardK k{};
    k.pt = make_point_dev(*point); k.log_w = log_w; k.n_ptr = n_valid; k.gathered = gathered;
    k.offs = offs; k.n0 = n0; k.lw_glob = lw_glob; k.anc = anc; k.flag = flag; k.lw_common = common;
    k.b = (long)b; k.D = dim; k.R = R; k.rank = rank;
    // 1. counts -> offsets, the global log-weight column
    const long pg = (cap + 255) / 256;
    hipLaunchKernelGGL(k_smc_shard_prefix, dim3((unsigned)(pg > 1024 ? 1024 : pg)), dim3(256), 0, st, k);
    // 2. the single-device decision on it
    SmcK d;
    d.log_w = lw_glob; d.n_ptr = n0; d.B = cap; d.tau = tau; d.u = u;
    d.cdf = cdf; d.anc = anc; d.flag = flag; d.lw_common = common;
    d.resampled_out = resampled; d.ess_out = ess; d.anc_out = ancestors; d.lw_pre_out = log_w_pre;
    FAB_TRY(smc_decide(d, st));
    // 3. this rank's rows fetch their ancestors
    const int grid = shard_grid((long)b);
    if (shard_vec_ok(*point, gathered, dim)) hipLaunchKernelGGL(k_smc_shard_gather<true>, dim3(grid), dim3(64 * SHARD_WAVES), 0, st, k);
    else hipLaunchKernelGGL(k_smc_shard_gather<false>, dim3(grid), dim3(64 * SHARD_WAVES), 0, st, k);
    return check_launch();
}

}  // extern "C"
