// The resamplers that keep a CDF in HBM: the torch-compatible float-CDF multinomial, and the fixed-point family - maximum,
// single-pass scan, multinomial and systematic search samplers.
//
// The resample path is HBM-bound integer/byte work: coalesced 16-byte loads, wave ballots and LDS
// partials, a single-pass decoupled-look-back prefix scan over fixed-point weights (integer sums are
// associative => bit-exact for any scan order), two-level binary search (tile prefixes, then inside
// one 4096-entry tile).  (The resamplers without a CDF: resample_emit.hip.)
#include "resample_device.h"
#include "resample_host.h"

#pragma clang fp contract(off)

namespace fab {

// ------------------------------------------------------------------------------------------------
// torch-compatible multinomial (sequential fp32 CDF, exactly the CPU kernel's arithmetic)
// ------------------------------------------------------------------------------------------------
// c[j] = fl32(c[j-1] + p[j]) is inherently serial (the rounding of every partial sum feeds the next one), and it
// is what torch's CPU multinomial computes.  One lane runs the add chain out of LDS (float4 at a time, ~6 cycles per
// element instead of a global-memory round trip per few elements); the second wave of the workgroup streams the
// next chunk in and the previous chunk's results out meanwhile (double buffer, one barrier per 2048 elements).
constexpr int SEQ_CH = 2048;

__global__ __launch_bounds__(128) void k_seq_cdf(const float* __restrict__ p, long n, float* __restrict__ c) {
    __shared__ __attribute__((aligned(16))) float buf[2][SEQ_CH];      // inputs  (double buffer)
    __shared__ __attribute__((aligned(16))) float res[2][SEQ_CH];      // results (separate: lets the reads run ahead)
    __shared__ float carry_sh;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long nch = (n + SEQ_CH - 1) / SEQ_CH;
    auto load_chunk = [&](long ch, float* dst) {
        const long base = ch * SEQ_CH;
        for (int i = lane; i < SEQ_CH; i += 64) dst[i] = (base + i < n) ? p[base + i] : 0.f;   // + 0.f is exact
    };
    auto store_chunk = [&](long ch, const float* src) {
        const long base = ch * SEQ_CH;
        for (int i = lane; i < SEQ_CH; i += 64)
            if (base + i < n) c[base + i] = src[i];
    };
    if (wave == 1 && nch > 0) load_chunk(0, buf[0]);
    if (tid == 0) carry_sh = 0.f;
    __syncthreads();
    for (long ch = 0; ch < nch; ++ch) {
        if (wave == 0) {
            if (lane == 0) {
                float s = carry_sh;
                const float4* __restrict__ vin = reinterpret_cast<const float4*>(buf[ch & 1]);
                float4* __restrict__ vout = reinterpret_cast<float4*>(res[ch & 1]);
#pragma unroll 8
                for (int j = 0; j < SEQ_CH / 4; ++j) {
                    float4 x = vin[j];
                    s += x.x; x.x = s;
                    s += x.y; x.y = s;
                    s += x.z; x.z = s;
                    s += x.w; x.w = s;
                    vout[j] = x;
                }
                carry_sh = s;
            }
        } else {
            if (ch > 0) store_chunk(ch - 1, res[(ch & 1) ^ 1]);
            if (ch + 1 < nch) load_chunk(ch + 1, buf[(ch & 1) ^ 1]);
        }
        __syncthreads();
    }
    if (wave == 1 && nch > 0) store_chunk(nch - 1, res[(nch - 1) & 1]);
    if (tid == 0) c[n] = carry_sh;   // total kept in the extra slot
}

__global__ void k_cdf_normalise(float* __restrict__ c, long n) {
    const float s = c[n];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float v = c[i] / s;
        if (i == n - 1) v = 1.f;
        c[i] = v;
    }
}

__global__ void k_search_f32cdf(const float* __restrict__ c, long n, const double* __restrict__ u, long ns,
                                long long* __restrict__ idx) {
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < ns; k += (long)gridDim.x * blockDim.x) {
        const double uk = u[k];
        long lo = 0, hi = n;
        while (hi - lo > 0) {
            const long mid = lo + (hi - lo) / 2;
            if ((double)c[mid] < uk) lo = mid + 1; else hi = mid;
        }
        idx[k] = lo;
    }
}

// ------------------------------------------------------------------------------------------------
// scalable fixed-point CDF:  q_i = floor(fl32(exp(fl64(w_i) - fl64(max))) * 2^36)
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 16;                         // per thread
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;   // 4096 weights per tile
constexpr unsigned long long FLAG_AGG = 1ull << 62, FLAG_INC = 2ull << 62, VAL_MASK = (1ull << 62) - 1ull;

struct ScanWs {          // workspace layout (all 256-byte aligned)
    float* max_part;             // [1024]
    float* max_val;              // [1]
    unsigned long long* desc;    // [ntiles] tile descriptors  (flag | value)
    unsigned int* ticket;        // [1] dynamic tile id
    unsigned long long* tile_inc;// [ntiles] inclusive prefix at the end of each tile
    unsigned long long* cdf;     // [n]
    unsigned long long* cdf16;   // [ceil(n / 16)] cdf16[g] = cdf[min(16 g + 15, n - 1)] (LDS scan only)
    unsigned long long* cdf256;  // [ceil(n / 256)] the same, every 256th value
    int variant;                 // store-pattern variant (A/B experiments)
    int want_sub;                // write cdf16 / cdf256 (only the multinomial sampler reads them)
};

__global__ __launch_bounds__(256) void k_max_partial(const float* __restrict__ lw, long n, float* __restrict__ part) {
    __shared__ float sh[256];
    float m = -INFINITY;
    const long n4 = (((size_t)lw & 15) == 0) ? (n >> 2) : 0;          // 16-byte vector body
    const float4* p4 = reinterpret_cast<const float4*>(lw);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const float4 v = p4[i];
        if (isfinite(v.x)) m = fmaxf(m, v.x);
        if (isfinite(v.y)) m = fmaxf(m, v.y);
        if (isfinite(v.z)) m = fmaxf(m, v.z);
        if (isfinite(v.w)) m = fmaxf(m, v.w);
    }
    for (long i = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = lw[i];
        if (isfinite(v)) m = fmaxf(m, v);
    }
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] = fmaxf(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void k_max_final(const float* __restrict__ part, int nblk, float* __restrict__ out) {
    __shared__ float sh[256];
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nblk; i += 256) m = fmaxf(m, part[i]);
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) sh[threadIdx.x] = fmaxf(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (sh[0] == -INFINITY) ? 0.f : sh[0];
}

// Single-pass inclusive scan with decoupled look-back.  One workgroup scans SCAN_BLOCK = 16384 weights
// (one dynamic ticket + one look-back per 16384 items: a single atomic word saturates at ~88 tickets/us);
// wave w owns search tile 4*blk + w (4096 consecutive weights) slab-wise — slab v = 256 consecutive
// weights, lane l owns 4 of them — so every global load/store instruction of a wave is a fully coalesced
// 1-2 KiB access.  Descriptors are 8-byte {flag,value} granules written/read with relaxed agent-scope
// atomics: the data IS the flag.
constexpr int SCAN_NW = 8;                              // waves per scan workgroup
constexpr int SCAN_WAVE_ITEMS = 2048;                   // weights per wave (half a search tile)
constexpr int SCAN_SLABS = SCAN_WAVE_ITEMS / 256;       // 8 slabs per wave
constexpr int SCAN_BLOCK = SCAN_WAVE_ITEMS * SCAN_NW;   // 16384 weights per workgroup / ticket

__global__ __launch_bounds__(64 * SCAN_NW) void k_scan_fixed(const float* __restrict__ lw, long n,
                                                             const float* __restrict__ max_val, ScanWs ws) {
    __shared__ unsigned long long wave_tot[SCAN_NW];
    __shared__ unsigned long long blk_prefix;
    __shared__ unsigned int blk_id_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) blk_id_sh = atomicAdd(ws.ticket, 1u);
    __syncthreads();
    const unsigned int blk = blk_id_sh;
    const long wbase = (long)blk * SCAN_BLOCK + (long)wave * SCAN_WAVE_ITEMS;
    const float mx = max_val[0];
    unsigned long long q[SCAN_SLABS][4];
    const bool vec = (wbase + SCAN_WAVE_ITEMS <= n) && (((size_t)lw & 15) == 0);
    if (vec) {
#pragma unroll
        for (int h = 0; h < SCAN_SLABS; h += 8) {          // 8 loads in flight per lane
            float4 x[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) x[v] = *reinterpret_cast<const float4*>(lw + wbase + (h + v) * 256 + lane * 4);
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                q[h + v][0] = fixed_weight(x[v].x, mx); q[h + v][1] = fixed_weight(x[v].y, mx);
                q[h + v][2] = fixed_weight(x[v].z, mx); q[h + v][3] = fixed_weight(x[v].w, mx);
            }
        }
    } else {
#pragma unroll
        for (int v = 0; v < SCAN_SLABS; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long i = wbase + v * 256 + lane * 4 + e;
                q[v][e] = (i < n) ? fixed_weight(lw[i], mx) : 0ull;
            }
    }
    // lane-local inclusive sums per slab, wave scan of the lane totals, running slab offsets
    unsigned long long excl[SCAN_SLABS];
    unsigned long long slab_off = 0ull;
#pragma unroll
    for (int v = 0; v < SCAN_SLABS; ++v) {
        q[v][1] += q[v][0]; q[v][2] += q[v][1]; q[v][3] += q[v][2];
        unsigned long long incl = q[v][3];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = shfl_up_u64(incl, off);
            if (lane >= off) incl += o;
        }
        excl[v] = slab_off + (incl - q[v][3]);
        slab_off += shfl_u64(incl, 63);
    }
    if (lane == 0) wave_tot[wave] = slab_off;      // wave (= search tile) total, identical in every lane
    __syncthreads();
    unsigned long long wave_off = 0ull, blk_tot = 0ull;
#pragma unroll
    for (int w = 0; w < SCAN_NW; ++w) { if (w < wave) wave_off += wave_tot[w]; blk_tot += wave_tot[w]; }
    // publish the aggregate, look back for the exclusive prefix (wave 0)
    if (wave == 0) {
        if (blk == 0) {
            if (lane == 0) {
                __hip_atomic_store(ws.desc + 0, FLAG_INC | blk_tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                blk_prefix = 0ull;
            }
        } else {
            if (lane == 0)
                __hip_atomic_store(ws.desc + blk, FLAG_AGG | blk_tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            unsigned long long ex = 0ull;
            long look = (long)blk - 1;
            while (true) {
                const long j = look - lane;
                unsigned long long d = 0ull;
                if (j >= 0) {
                    do {
                        d = __hip_atomic_load(ws.desc + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } while ((d >> 62) == 0ull);
                } else {
                    d = FLAG_INC;          // virtual block before the first: inclusive prefix 0
                }
                const unsigned long long inc_mask = __ballot((d >> 62) == 2ull);
                const int first_inc = __ffsll((long long)inc_mask) - 1;
                unsigned long long contrib = (first_inc < 0 || lane <= first_inc) ? (d & VAL_MASK) : 0ull;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) contrib += shfl_u64(contrib, lane ^ off);
                ex += contrib;
                if (first_inc >= 0) break;
                look -= 64;
            }
            if (lane == 0) {
                __hip_atomic_store(ws.desc + blk, FLAG_INC | (ex + blk_tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                blk_prefix = ex;
            }
        }
    }
    __syncthreads();
    const unsigned long long off0 = blk_prefix + wave_off;
    // inclusive prefix at the end of every 4096-weight search tile (= two waves)
    if (lane == 63 && (wave & 1) && wbase - SCAN_WAVE_ITEMS < n)
        ws.tile_inc[((long)blk * SCAN_BLOCK + (long)(wave - 1) * SCAN_WAVE_ITEMS) / SCAN_TILE] = off0 + slab_off;
    if (vec && ws.variant == 1) {
        // fully contiguous 1-KiB store instructions: lane j stores items (2j, 2j+1) of each half slab, which
        // live in lane j/2 (first half) / 32 + j/2 (second half) -> one lane exchange per value
        const int srcA = lane >> 1, srcB = 32 + (lane >> 1);
        const bool odd = lane & 1;
#pragma unroll
        for (int v = 0; v < SCAN_SLABS; ++v) {
            const unsigned long long b = off0 + excl[v];
            const unsigned long long c0 = b + q[v][0], c1 = b + q[v][1], c2 = b + q[v][2], c3 = b + q[v][3];
            const unsigned long long lo = odd ? c2 : c0, hi = odd ? c3 : c1;   // what a consumer of MY data wants
            // consumer lane j reads from lane src; the value it needs depends on ITS parity, so send both pairs
            const unsigned long long a0 = shfl_u64(c0, srcA), a1 = shfl_u64(c1, srcA), a2 = shfl_u64(c2, srcA), a3 = shfl_u64(c3, srcA);
            const unsigned long long b0 = shfl_u64(c0, srcB), b1 = shfl_u64(c1, srcB), b2 = shfl_u64(c2, srcB), b3 = shfl_u64(c3, srcB);
            (void)lo; (void)hi;
            ulonglong2* oA = reinterpret_cast<ulonglong2*>(ws.cdf + wbase + v * 256 + lane * 2);
            ulonglong2* oB = reinterpret_cast<ulonglong2*>(ws.cdf + wbase + v * 256 + 128 + lane * 2);
            *oA = odd ? make_ulonglong2(a2, a3) : make_ulonglong2(a0, a1);
            *oB = odd ? make_ulonglong2(b2, b3) : make_ulonglong2(b0, b1);
        }
    } else if (vec && ws.variant == 2) {
        // same pattern, streaming (non-temporal) stores: the CDF is consumed by a later kernel, not by this one
        typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
        const int srcA = lane >> 1, srcB = 32 + (lane >> 1);
        const bool odd = lane & 1;
#pragma unroll
        for (int v = 0; v < SCAN_SLABS; ++v) {
            const unsigned long long b = off0 + excl[v];
            const unsigned long long c0 = b + q[v][0], c1 = b + q[v][1], c2 = b + q[v][2], c3 = b + q[v][3];
            const unsigned long long a0 = shfl_u64(c0, srcA), a1 = shfl_u64(c1, srcA), a2 = shfl_u64(c2, srcA), a3 = shfl_u64(c3, srcA);
            const unsigned long long b0 = shfl_u64(c0, srcB), b1 = shfl_u64(c1, srcB), b2 = shfl_u64(c2, srcB), b3 = shfl_u64(c3, srcB);
            u64x2* oA = reinterpret_cast<u64x2*>(ws.cdf + wbase + v * 256 + lane * 2);
            u64x2* oB = reinterpret_cast<u64x2*>(ws.cdf + wbase + v * 256 + 128 + lane * 2);
            const u64x2 vA = odd ? (u64x2){a2, a3} : (u64x2){a0, a1};
            const u64x2 vB = odd ? (u64x2){b2, b3} : (u64x2){b0, b1};
            __builtin_nontemporal_store(vA, oA);
            __builtin_nontemporal_store(vB, oB);
        }
    } else if (vec) {
#pragma unroll
        for (int v = 0; v < SCAN_SLABS; ++v) {
            ulonglong2* o2 = reinterpret_cast<ulonglong2*>(ws.cdf + wbase + v * 256 + lane * 4);
            const unsigned long long b = off0 + excl[v];
            o2[0] = make_ulonglong2(b + q[v][0], b + q[v][1]);
            o2[1] = make_ulonglong2(b + q[v][2], b + q[v][3]);
        }
    } else {
#pragma unroll
        for (int v = 0; v < SCAN_SLABS; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long i = wbase + v * 256 + lane * 4 + e;
                if (i < n) ws.cdf[i] = off0 + excl[v] + q[v][e];
            }
    }
}

// Same scan, LDS-transposed: the wave's 2048 weights are loaded with fully coalesced 1-KiB instructions, turned
// in LDS so that lane l owns the 32 CONSECUTIVE weights [32 l, 32 l + 32), summed serially in registers (one
// 6-step wave scan per 2048 weights instead of one per 256), and the 2048 CDF values are turned back through
// LDS into fully coalesced non-temporal 1-KiB stores.  Integer sums: bit-identical to k_scan_fixed.
// LDS per wave: 64 lanes x 18 u64 (the CDF goes back in two halves of 16 values per lane; lane stride 144 B);
// the float staging of the input (lane stride 36 floats = 144 B) aliases the same region.  73 KB per
// workgroup -> two workgroups per CU.
constexpr int SCAN_LSTRIDE = 18;                        // u64 per lane row (16 + 2 pad)
constexpr int SCAN_FSTRIDE = 36;                        // floats per lane row of the input staging

__global__ __launch_bounds__(64 * SCAN_NW) void k_scan_fixed_lds(const float* __restrict__ lw, long n,
                                                                 const float* __restrict__ max_val, ScanWs ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long scan_lds[];
    __shared__ unsigned long long wave_tot[SCAN_NW];
    __shared__ unsigned long long blk_prefix;
    __shared__ unsigned int blk_id_sh;
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) blk_id_sh = atomicAdd(ws.ticket, 1u);
    __syncthreads();
    const unsigned int blk = blk_id_sh;
    const long wbase = (long)blk * SCAN_BLOCK + (long)wave * SCAN_WAVE_ITEMS;
    const float mx = max_val[0];
    unsigned long long* wl = scan_lds + (size_t)wave * 64 * SCAN_LSTRIDE;
    float* wf = reinterpret_cast<float*>(wl);
    const bool vec = (wbase + SCAN_WAVE_ITEMS <= n) && (((size_t)lw & 15) == 0);
    unsigned long long run[32];                          // inclusive sums of this lane's 32 consecutive weights
    if (vec) {
        float4 x[8];
#pragma unroll
        for (int h = 0; h < 8; ++h) x[h] = *reinterpret_cast<const float4*>(lw + wbase + h * 256 + lane * 4);
#pragma unroll
        for (int h = 0; h < 8; ++h)                      // item 256 h + 4 lane -> row (8 h + lane / 8), column 4 (lane % 8)
            *reinterpret_cast<float4*>(wf + (8 * h + (lane >> 3)) * SCAN_FSTRIDE + 4 * (lane & 7)) = x[h];
    } else {
        for (int i = lane; i < SCAN_WAVE_ITEMS; i += 64) {
            const long g = wbase + i;
            wf[(i >> 5) * SCAN_FSTRIDE + (i & 31)] = (g < n) ? lw[g] : -INFINITY;
        }
    }
    __builtin_amdgcn_wave_barrier();
    unsigned long long acc = 0ull;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 y = *reinterpret_cast<const float4*>(wf + lane * SCAN_FSTRIDE + 4 * k);
        acc += fixed_weight(y.x, mx); run[4 * k + 0] = acc;
        acc += fixed_weight(y.y, mx); run[4 * k + 1] = acc;
        acc += fixed_weight(y.z, mx); run[4 * k + 2] = acc;
        acc += fixed_weight(y.w, mx); run[4 * k + 3] = acc;
    }
    unsigned long long incl = acc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = shfl_up_u64(incl, off);
        if (lane >= off) incl += o;
    }
    const unsigned long long lane_excl = incl - acc;
    const unsigned long long wtot = shfl_u64(incl, 63);
    if (lane == 0) wave_tot[wave] = wtot;
    __syncthreads();
    unsigned long long wave_off = 0ull, blk_tot = 0ull;
#pragma unroll
    for (int w = 0; w < SCAN_NW; ++w) { if (w < wave) wave_off += wave_tot[w]; blk_tot += wave_tot[w]; }
    if (wave == 0) {
        if (blk == 0) {
            if (lane == 0) {
                __hip_atomic_store(ws.desc + 0, FLAG_INC | blk_tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                blk_prefix = 0ull;
            }
        } else {
            if (lane == 0)
                __hip_atomic_store(ws.desc + blk, FLAG_AGG | blk_tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            unsigned long long ex = 0ull;
            long look = (long)blk - 1;
            while (true) {
                const long j = look - lane;
                unsigned long long d = 0ull;
                if (j >= 0) {
                    do {
                        d = __hip_atomic_load(ws.desc + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } while ((d >> 62) == 0ull);
                } else {
                    d = FLAG_INC;
                }
                const unsigned long long inc_mask = __ballot((d >> 62) == 2ull);
                const int first_inc = __ffsll((long long)inc_mask) - 1;
                unsigned long long contrib = (first_inc < 0 || lane <= first_inc) ? (d & VAL_MASK) : 0ull;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) contrib += shfl_u64(contrib, lane ^ off);
                ex += contrib;
                if (first_inc >= 0) break;
                look -= 64;
            }
            if (lane == 0) {
                __hip_atomic_store(ws.desc + blk, FLAG_INC | (ex + blk_tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                blk_prefix = ex;
            }
        }
    }
    __syncthreads();
    const unsigned long long off0 = blk_prefix + wave_off;
    if (lane == 63 && (wave & 1) && wbase - SCAN_WAVE_ITEMS < n)
        ws.tile_inc[((long)blk * SCAN_BLOCK + (long)(wave - 1) * SCAN_WAVE_ITEMS) / SCAN_TILE] = off0 + wtot;
    const unsigned long long base = off0 + lane_excl;
    if (ws.want_sub) {                                   // sub-sampled CDF: the last value of each 16-group (padding weighs 0)
        const long g0 = (wbase + 32 * lane) >> 4;
        if ((g0 << 4) < n) ws.cdf16[g0] = base + run[15];
        if (((g0 + 1) << 4) < n) ws.cdf16[g0 + 1] = base + run[31];
        if ((lane & 7) == 7 && wbase + 32 * (lane - 7) < n) ws.cdf256[(wbase + 32 * lane) >> 8] = base + run[31];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {                        // values 16 h .. 16 h + 15 of every lane
#pragma unroll
        for (int k = 0; k < 8; ++k)
            *reinterpret_cast<u64x2*>(wl + lane * SCAN_LSTRIDE + 2 * k) =
                (u64x2){base + run[16 * h + 2 * k], base + run[16 * h + 2 * k + 1]};
        __builtin_amdgcn_wave_barrier();
        if (vec) {
#pragma unroll
            for (int s = 0; s < 8; ++s) {                // 8 lanes write one full 128-byte line of row 8 s + lane / 8
                const int row = 8 * s + (lane >> 3), col = 2 * (lane & 7);
                const u64x2 c = *reinterpret_cast<const u64x2*>(wl + row * SCAN_LSTRIDE + col);
                __builtin_nontemporal_store(c, reinterpret_cast<u64x2*>(ws.cdf + wbase + 32 * row + 16 * h + col));
            }
        } else {
            for (int i = lane; i < SCAN_WAVE_ITEMS / 2; i += 64) {
                const long g = wbase + 32 * (i >> 4) + 16 * h + (i & 15);
                if (g < n) ws.cdf[g] = wl[(i >> 4) * SCAN_LSTRIDE + (i & 15)];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// first j with C[j] > t : search the tile prefixes, then inside the tile
__device__ __forceinline__ long search_cdf(const ScanWs& ws, long n, long ntiles, unsigned long long t) {
    long lo = 0, hi = ntiles;
    while (lo < hi) { const long mid = (lo + hi) >> 1; if (ws.tile_inc[mid] > t) hi = mid; else lo = mid + 1; }
    if (lo >= ntiles) return n - 1;
    long a = lo * SCAN_TILE, b = a + SCAN_TILE;
    if (b > n) b = n;
    while (a < b) { const long mid = (a + b) >> 1; if (ws.cdf[mid] > t) b = mid; else a = mid + 1; }
    return a < n ? a : n - 1;
}

// Multinomial sampler: the thresholds are unordered, so every draw walks the CDF on its own.  A bisection of a 4096-entry
// tile of the full CDF touches 9 distinct cache lines of an 8N-byte array per draw, and - with thousands of searches in
// flight per CU - even the last steps inside one line miss the 32 KB L1 again (measured: splitting the tile search over
// sub-sampled tables cut the time only from 9.6 to 5.1 ms at N = 2^26, more searches in flight per thread made it slower).
// So below the tile the search is 16-ary over three tables the LDS scan writes - cdf256 (every 256th value, N/32 bytes,
// L2-resident), cdf16 (N/2 bytes, MALL), the CDF itself - and each 16-entry node is ONE 128-byte line fetched ONCE by a
// group of 8 lanes (16 bytes each, coalesced); the position inside the node is a ballot + popcount.  A wave serves its
// 64 draws in 8 rounds (group g, round r: the draw of lane 8 g + r), all 8 rounds of a level in flight together.
// The tile prefixes are one more 16-ary level; above it the last prefix of every `cs`-th 16-tile node (<= 4096 entries,
// cs = 1 up to N = 2^28) is bisected in LDS.
constexpr int MN_COARSE = 4096;

// one 16-ary level for the wave's 8 rounds: p[r] (node start, multiple of 16) += entries <= t among the node's 16
__device__ __forceinline__ void node16_level(const unsigned long long* __restrict__ table, long len, long (&p)[8],
                                             const unsigned long long (&t)[8], int sub, int gbase) {
    ulonglong2 v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = *reinterpret_cast<const ulonglong2*>(table + p[r] + 2 * sub);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const long i0 = p[r] + 2 * sub;
        const unsigned long long bx = __ballot(i0 < len && v[r].x <= t[r]);
        const unsigned long long by = __ballot(i0 + 1 < len && v[r].y <= t[r]);
        p[r] += __popc((unsigned)((bx >> gbase) & 0xffull)) + __popc((unsigned)((by >> gbase) & 0xffull));
    }
}

__global__ __launch_bounds__(256) void k_sample_multinomial(ScanWs ws, long n, long ntiles, const double* __restrict__ u,
                                                            long ns, long long* __restrict__ idx) {
    __shared__ unsigned long long coarse[MN_COARSE];
    const unsigned long long total = ws.tile_inc[ntiles - 1];
    if (ws.variant != 3) {                           // only the LDS scan writes the sub-sampled tables
        for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < ns; k += (long)gridDim.x * blockDim.x) {
            unsigned long long t = 0ull;
            if (total > 0ull) {
                t = (unsigned long long)floor(u[k] * (double)total);
                if (t > total - 1ull) t = total - 1ull;
            }
            idx[k] = search_cdf(ws, n, ntiles, t);
        }
        return;
    }
    // LDS: the inclusive prefix at the end of every `cs`-th 16-tile node (cs = 1 up to N = 2^28)
    const long nnodes = (ntiles + 15) >> 4;
    const long cs = (nnodes + MN_COARSE - 1) / MN_COARSE, nc = (nnodes + cs - 1) / cs;
    for (long i = threadIdx.x; i < nc; i += blockDim.x) {
        const long j = 16 * (i + 1) * cs - 1;
        coarse[i] = ws.tile_inc[j < ntiles ? j : ntiles - 1];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, sub = lane & 7, gbase = lane & ~7;
    const long n256 = (n + 255) >> 8, n16 = (n + 15) >> 4;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long w0 = (long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); w0 < ns; w0 += stride) {   // wave-uniform trip count
        const long k = w0 + lane;
        unsigned long long t = 0ull;
        if (k < ns && total > 0ull) {
            t = (unsigned long long)floor(u[k] * (double)total);
            if (t > total - 1ull) t = total - 1ull;
        }
        // this lane's 16-tile node: first node whose last inclusive prefix exceeds t
        long lo = 0, hi = nc;
        while (lo < hi) { const long mid = (lo + hi) >> 1; if (coarse[mid] > t) hi = mid; else lo = mid + 1; }
        lo *= cs; hi = lo + cs;
        if (hi > nnodes) hi = nnodes;
        while (lo < hi) {
            const long mid = (lo + hi) >> 1, j = 16 * mid + 15;
            if (ws.tile_inc[j < ntiles ? j : ntiles - 1] > t) hi = mid; else lo = mid + 1;
        }
        if (lo > nnodes - 1) lo = nnodes - 1;        // (only when total == 0)
        long p[8];
        unsigned long long tr[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            tr[r] = shfl_u64(t, gbase + r);
            p[r] = shfl_i64(lo, gbase + r) << 4;
        }
        node16_level(ws.tile_inc, ntiles, p, tr, sub, gbase);
#pragma unroll
        for (int r = 0; r < 8; ++r) p[r] = (p[r] < ntiles ? p[r] : ntiles - 1) * (SCAN_TILE / 256);
        node16_level(ws.cdf256, n256, p, tr, sub, gbase);
#pragma unroll
        for (int r = 0; r < 8; ++r) p[r] = (p[r] < n256 ? p[r] : n256 - 1) << 4;
        node16_level(ws.cdf16, n16, p, tr, sub, gbase);
#pragma unroll
        for (int r = 0; r < 8; ++r) p[r] = (p[r] < n16 ? p[r] : n16 - 1) << 4;
        node16_level(ws.cdf, n, p, tr, sub, gbase);
        long res = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) res = sub == r ? p[r] : res;
        if (k < ns) idx[k] = (total > 0ull && res < n) ? res : n - 1;
    }
}

// Systematic thresholds are sorted, so a chunk of 4096 consecutive samples lands in a short run of CDF
// tiles: stage each tile (32 KiB) in LDS and binary-search there -> indices are written coalesced and the
// work is balanced in SAMPLES whatever the weight distribution (a tile-driven variant was 1.75x slower on
// heavy-tailed weights).  Chunks that span many (near-empty) tiles fall back to the global two-level search;
// the total number of staged tiles is bounded by ntiles + nchunks.
constexpr int SYS_CHUNK = 4096, SYS_PER_THREAD = SYS_CHUNK / 256, SYS_MAX_SPAN = 8;

__global__ __launch_bounds__(256) void k_sample_systematic(ScanWs ws, long n, long ntiles,
                                                           const unsigned long long* __restrict__ strata_ptr, long ns,
                                                           long long* __restrict__ idx) {
    __shared__ unsigned long long cdf_sh[SCAN_TILE];
    __shared__ long span_sh[2];
    const int tid = threadIdx.x;
    const Strata sm = load_strata(strata_ptr);
    const unsigned long long total = sm.total;
    const long k0 = (long)blockIdx.x * SYS_CHUNK;
    unsigned long long t[SYS_PER_THREAD];
#pragma unroll
    for (int m = 0; m < SYS_PER_THREAD; ++m) {
        const long k = k0 + tid + 256 * m;
        t[m] = (total > 0ull && k < ns) ? ((unsigned long long)k * sm.S + sm.U) >> sm.F : 0ull;
    }
    if (tid == 0) {                 // first / last tile touched by this chunk (thresholds are monotone in k)
        const long kl = (k0 + SYS_CHUNK <= ns ? k0 + SYS_CHUNK : ns) - 1;
        const unsigned long long tl = total > 0ull ? ((unsigned long long)kl * sm.S + sm.U) >> sm.F : 0ull;
        long lo = 0, hi = ntiles;
        while (lo < hi) { const long mid = (lo + hi) >> 1; if (ws.tile_inc[mid] > t[0]) hi = mid; else lo = mid + 1; }
        span_sh[0] = lo < ntiles ? lo : ntiles - 1;
        lo = 0; hi = ntiles;
        while (lo < hi) { const long mid = (lo + hi) >> 1; if (ws.tile_inc[mid] > tl) hi = mid; else lo = mid + 1; }
        span_sh[1] = lo < ntiles ? lo : ntiles - 1;
    }
    __syncthreads();
    const long ta = span_sh[0], tb = span_sh[1];
    if (tb - ta + 1 > SYS_MAX_SPAN) {
#pragma unroll
        for (int m = 0; m < SYS_PER_THREAD; ++m) {
            const long k = k0 + tid + 256 * m;
            if (k < ns) idx[k] = search_cdf(ws, n, ntiles, t[m]);
        }
        return;
    }
    unsigned done = 0u;
    for (long tile = ta; tile <= tb; ++tile) {
        const long base = tile * SCAN_TILE;
        const long len = (base + SCAN_TILE <= n) ? SCAN_TILE : n - base;
        for (int i = tid * 2; i < SCAN_TILE; i += 512) {
            if (i + 1 < len) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(ws.cdf + base + i);
                cdf_sh[i] = v.x; cdf_sh[i + 1] = v.y;
            } else {
                cdf_sh[i] = (i < len) ? ws.cdf[base + i] : ~0ull;
                cdf_sh[i + 1] = ~0ull;
            }
        }
        __syncthreads();
        const unsigned long long c_end = ws.tile_inc[tile];
#pragma unroll
        for (int m = 0; m < SYS_PER_THREAD; ++m) {
            const long k = k0 + tid + 256 * m;
            if (k < ns && !((done >> m) & 1u) && (t[m] < c_end || tile == tb)) {
                int a = 0, b = (int)len;
                while (a < b) { const int mid = (a + b) >> 1; if (cdf_sh[mid] > t[m]) b = mid; else a = mid + 1; }
                long r = base + a;
                idx[k] = r < n ? r : n - 1;
                done |= 1u << m;
            }
        }
        __syncthreads();
    }
}

// stratum map for the scan + search path (total = last tile prefix)
__global__ void k_strata_params(const unsigned long long* __restrict__ total_ptr, double u0, long ns,
                                unsigned long long* __restrict__ strata_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const Strata m = make_strata(*total_ptr, u0, ns);
    strata_out[0] = m.total; strata_out[1] = m.S; strata_out[2] = m.U; strata_out[3] = (unsigned long long)m.F;
}

static inline long scan_tiles(long n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

static ScanWs carve_scan_ws(void* workspace, long n) {
    char* p = (char*)workspace;
    ScanWs ws;
    ws.max_part = (float*)p; p += al256(1024 * 4);
    ws.max_val = (float*)p; p += 256;
    ws.desc = (unsigned long long*)p; p += al256((size_t)scan_tiles(n) * 8);
    ws.ticket = (unsigned int*)p; p += 256;
    ws.tile_inc = (unsigned long long*)p; p += al256((size_t)scan_tiles(n) * 8);
    ws.cdf = (unsigned long long*)p; p += al256((size_t)n * 8);
    ws.cdf16 = (unsigned long long*)p; p += al256(((size_t)n / 16 + 1) * 8);
    ws.cdf256 = (unsigned long long*)p;
    ws.want_sub = 0;
    ws.variant = option(FABHIP_OPT_SCAN_VARIANT);   // 3 = LDS-transposed scan; 0-2 = register/shuffle variants (A/B)
    return ws;
}

void scan_ws_regions(void* workspace, long n, float** max_part, float** max_val, unsigned long long** cdf) {
    const ScanWs ws = carve_scan_ws(workspace, n);
    *max_part = ws.max_part; *max_val = ws.max_val; *cdf = ws.cdf;
}

void launch_max(const float* log_w, long n, float* max_part, float* max_val, hipStream_t st) {
    const int mb = grid_for(n, 256 * 16, 1024);
    hipLaunchKernelGGL(k_max_partial, dim3(mb), dim3(256), 0, st, log_w, n, max_part);
    hipLaunchKernelGGL(k_max_final, dim3(1), dim3(256), 0, st, max_part, mb, max_val);
}

static int build_fixed_cdf(const float* log_w, long n, const ScanWs& ws, hipStream_t st, bool reuse_max = false) {
    if (!reuse_max) launch_max(log_w, n, ws.max_part, ws.max_val, st);
    // zero descriptors + ticket (one contiguous region: desc .. ticket)
    const size_t zbytes = (size_t)((char*)ws.ticket - (char*)ws.desc) + 256;
    if (hipMemsetAsync(ws.desc, 0, zbytes, st) != hipSuccess) return FABHIP_ELAUNCH;
    const dim3 grid((unsigned)((n + SCAN_BLOCK - 1) / SCAN_BLOCK)), block(64 * SCAN_NW);
    if (ws.variant == 3) {
        const size_t lds = (size_t)SCAN_NW * 64 * SCAN_LSTRIDE * sizeof(unsigned long long);
        FAB_TRY(set_max_lds((const void*)k_scan_fixed_lds, lds));
        hipLaunchKernelGGL(k_scan_fixed_lds, grid, block, lds, st, log_w, n, ws.max_val, ws);
    } else {
        hipLaunchKernelGGL(k_scan_fixed, grid, block, 0, st, log_w, n, ws.max_val, ws);
    }
    return check_launch();
}

int systematic_by_search(const float* log_w, long n, double u0, long ns, long long* idx, void* workspace, hipStream_t st) {
    const ScanWs ws = carve_scan_ws(workspace, n);
    FAB_TRY(build_fixed_cdf(log_w, n, ws, st));
    unsigned long long* strata = ws.desc;                    // the descriptors are dead once the scan is done
    hipLaunchKernelGGL(k_strata_params, dim3(1), dim3(1), 0, st, ws.tile_inc + (scan_tiles(n) - 1), u0, ns, strata);
    hipLaunchKernelGGL(k_sample_systematic, dim3((unsigned)((ns + SYS_CHUNK - 1) / SYS_CHUNK)), dim3(256), 0, st, ws, n,
                       scan_tiles(n), strata, ns, idx);
    return check_launch();
}

}  // namespace fab

using namespace fab;

extern "C" {

size_t fabhip_multinomial_torch_workspace_bytes(int64_t n) { return al256((size_t)(n + 1) * 4) + 256; }

int fabhip_multinomial_torch(const float* probs, int64_t n, const double* u, int64_t n_samples, int64_t* idx,
                             void* workspace, size_t workspace_bytes, fabhip_stream_t stream) {
    if (!probs || !u || !idx || !workspace || n < 1 || n_samples < 0) return FABHIP_EINVAL;
    if (workspace_bytes < fabhip_multinomial_torch_workspace_bytes(n)) return FABHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    float* c = (float*)workspace;
    hipLaunchKernelGGL(k_seq_cdf, dim3(1), dim3(128), 0, st, probs, (long)n, c);
    hipLaunchKernelGGL(k_cdf_normalise, dim3(grid_for(n, 256, 2048)), dim3(256), 0, st, c, (long)n);
    if (n_samples > 0)
        hipLaunchKernelGGL(k_search_f32cdf, dim3(grid_for(n_samples, 256, 4096)), dim3(256), 0, st, c, (long)n, u,
                           (long)n_samples, (long long*)idx);
    return check_launch();
}

size_t fabhip_resample_workspace_bytes(int64_t n) {
    const size_t tiles = (size_t)scan_tiles(n);
    return al256(1024 * 4) + 256 + al256(tiles * 8) + 256 + al256(tiles * 8) + al256((size_t)n * 8) +
           al256(((size_t)n / 16 + 1) * 8) + al256(((size_t)n / 256 + 1) * 8) + 256;
}

int fabhip_fixed_cdf(const float* log_w, int64_t n, int32_t reuse_max, const uint64_t** cdf_out, void* workspace,
                     size_t workspace_bytes, fabhip_stream_t stream) {
    if (!log_w || !workspace || n < 1) return FABHIP_EINVAL;
    if (((size_t)workspace & 255) != 0) return FABHIP_EINVAL;
    if (workspace_bytes < fabhip_resample_workspace_bytes(n)) return FABHIP_ENOSPC;
    const ScanWs ws = carve_scan_ws(workspace, n);
    if (cdf_out) *cdf_out = (const uint64_t*)ws.cdf;
    return build_fixed_cdf(log_w, n, ws, (hipStream_t)stream, reuse_max != 0);
}

int fabhip_resample_multinomial(const float* log_w, int64_t n, const double* u, int64_t n_samples, int64_t* idx,
                                void* workspace, size_t workspace_bytes, fabhip_stream_t stream) {
    if (!log_w || !u || !idx || !workspace || n < 1 || n_samples < 0) return FABHIP_EINVAL;
    if (((size_t)workspace & 255) != 0) return FABHIP_EINVAL;
    if (workspace_bytes < fabhip_resample_workspace_bytes(n)) return FABHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    ScanWs ws = carve_scan_ws(workspace, n);
    ws.want_sub = 1;
    FAB_TRY(build_fixed_cdf(log_w, n, ws, st));
    if (n_samples > 0)
        hipLaunchKernelGGL(k_sample_multinomial, dim3(grid_for(n_samples, 256, 4096)), dim3(256), 0, st, ws, (long)n,
                           scan_tiles(n), u, (long)n_samples, (long long*)idx);
    return check_launch();
}

}  // extern "C"
