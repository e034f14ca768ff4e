// The resamplers that keep no CDF in HBM: every wave re-derives the CDF of its 1024 weights in registers and EMITS the indices
// its weights own - systematic, stratified (k_emit_*) and the seeded streaming multinomial (k_ms_*).  One host path for the
// three (EmitWs, emit_front, emit_finish) at the end of the file.
#include "resample_device.h"
#include "resample_host.h"

#pragma clang fp contract(off)

namespace fab {

// ------------------------------------------------------------------------------------------------
// Systematic resampling.  Stratum map (oracle/numerical.py:systematic_strata restates it): pure 64-bit integers
//     F = 62 - bit_length(total),  S = floor(total 2^F / ns),  U = min(floor(u0 S), S - 1),   t_k = (k S + U) >> F
// i.e. ns equal strata of width S / 2^F offset by u0 strata.  Its inverse, "the first stratum whose threshold
// reaches C", is K(C) = ceil(((C << F) - U) / S), evaluated as a float64 estimate + ONE exact integer correction step.
//
// Fused path (no CDF in HBM, no per-stratum search):
//   pass T  k_emit_wave_sums : fixed-point weight sum of every 1024-weight wave tile + of every 4096-weight block (EM_NW waves)
//           k_emit_prefix    : exclusive prefix over the block sums (one workgroup), total, (F, S, U)      (reads 4N)
//   pass E  k_emit_systematic: every wave re-derives the CDF of its 1024 weights in registers (coalesced loads, LDS
//           transpose so that a lane owns 16 consecutive weights, serial sums + one 6-step wave scan).  Weight j owns the
//           CONTIGUOUS strata [K(C_{j-1}), K(C_j)): the resampled index array is an EXPANSION - weight j repeated
//           K(C_j) - K(C_{j-1}) times.  Every weight with a non-empty run drops ONE marker (its id) at the first
//           position of its run in a 1536-entry LDS window; an inclusive max-scan (ids grow with position) fills the
//           runs - no data-dependent loop, no divergence, a heavy weight costs nothing extra - and the window is
//           flushed with coalesced 32-byte-per-lane stores.  Runs >= 32768 strata (all the mass on a few particles)
//           are published and filled by a grid-wide kernel instead of one wave.                 (reads 4N, writes 8 ns)
// Integer prefix sums and an exact inverse => bit-identical to the scan + search path and to the oracle.
// HBM traffic 12N + 8 ns bytes instead of 4N + 12N + 16 ns.
// ------------------------------------------------------------------------------------------------
constexpr int EM_NW = 4;                                // waves per workgroup (r4: 4 x 7 KiB of LDS -> 5 workgroups = 20 waves per CU at <= 96
                                                        // VGPRs, was 8 waves x 9 KiB -> 16 per CU: 402 -> 382 us end to end at 2^26)
constexpr int EM_WAVE_ITEMS = 1024;                     // weights per wave: 16 consecutive per lane
constexpr int EM_BLOCK = EM_WAVE_ITEMS * EM_NW;
constexpr int EM_FSTRIDE = 20;                          // floats per lane row of the input staging (16 + 4 pad)
constexpr int EM_WIN = 1536;                            // int32 marker window (entries) per wave: EM_ROW = 24 per lane row (a wave owns ~1024
                                                        // strata when ns = N; 1024 entries: two passes for half the waves, 402 us)
constexpr int EM_WSTRIDE = 28;                          // dwords per lane row of the window (24 + 4 pad: 28 i mod 64 distinct multiples of 4
                                                        // over 16 lanes: conflict-free b128)
constexpr int EM_WAVE_LDS = 64 * EM_WSTRIDE * 4;        // bytes per wave (>= 64 * EM_FSTRIDE * 4)
constexpr int EM_ROW = EM_WIN / 64;                     // window entries per lane row
__device__ __forceinline__ int em_waddr(int e) { const int r = (int)((unsigned)e / (unsigned)EM_ROW); return r * EM_WSTRIDE + (e - r * EM_ROW); }
constexpr int EM_GIANT = 32768;                         // runs at least this long are filled by a grid-wide kernel

__global__ __launch_bounds__(64 * EM_NW) void k_emit_wave_sums(const float* __restrict__ lw, long n,
                                                               const float* __restrict__ max_val,
                                                               unsigned long long* __restrict__ wave_sum,
                                                               unsigned long long* __restrict__ block_sum) {
    __shared__ unsigned long long wsum[EM_NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long wt = (long)blockIdx.x * EM_NW + wave;
    const long wbase = wt * EM_WAVE_ITEMS;
    const float mx = max_val[0];
    unsigned long long acc = 0ull;
    if (wbase + EM_WAVE_ITEMS <= n && (((size_t)lw & 15) == 0)) {
        float4 x[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) x[h] = *reinterpret_cast<const float4*>(lw + wbase + h * 256 + lane * 4);
#pragma unroll
        for (int h = 0; h < 4; ++h)
            acc += fixed_weight(x[h].x, mx) + fixed_weight(x[h].y, mx) + fixed_weight(x[h].z, mx) + fixed_weight(x[h].w, mx);
    } else {
        for (int i = lane; i < EM_WAVE_ITEMS; i += 64)
            if (wbase + i < n) acc += fixed_weight(lw[wbase + i], mx);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += shfl_u64(acc, lane ^ off);
    if (lane == 0) { wsum[wave] = acc; if (wbase < n) wave_sum[wt] = acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = 0ull;
        for (int w = 0; w < EM_NW; ++w) b += wsum[w];
        block_sum[blockIdx.x] = b;
    }
}

// exclusive prefix over the block sums (nb = ceil(N / EM_BLOCK)): one 1024-thread workgroup, a contiguous chunk per thread;
// also the stratum map {total, S, U, F} and the reset of the giant-run counter
__global__ __launch_bounds__(1024) void k_emit_prefix(const unsigned long long* __restrict__ block_sum, long nb,
                                                      unsigned long long* __restrict__ block_excl, double u0, long ns,
                                                      unsigned long long* __restrict__ strata_out,
                                                      unsigned long long* __restrict__ giant_count) {
    __shared__ unsigned long long part[1024];
    const int tid = threadIdx.x;
    if (tid == 0) *giant_count = 0ull;
    const long chunk = (nb + 1023) / 1024;
    const long a = (long)tid * chunk, b = a + chunk < nb ? a + chunk : nb;
    unsigned long long s = 0ull;
    for (long i = a; i < b; ++i) s += block_sum[i];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {               // Hillis-Steele inclusive scan of the chunk sums
        const unsigned long long v = tid >= off ? part[tid - off] : 0ull;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    unsigned long long run = tid ? part[tid - 1] : 0ull;
    for (long i = a; i < b; ++i) { block_excl[i] = run; run += block_sum[i]; }
    if (tid == 1023) {
        const Strata m = make_strata(part[1023], u0, ns);
        strata_out[0] = m.total; strata_out[1] = m.S; strata_out[2] = m.U; strata_out[3] = (unsigned long long)m.F;
    }
}

// K(C) - Kref for a CDF value C = c0 + d (d < 2^47), as int32: float64 estimate of ceil(((C << F) - U) / S) with
// num0 = (double)((c0 << F) - U) (signed) supplied by the caller, then one exact integer correction step
// (estimate error << 1 stratum: the conversions lose < 2^-26 of a stratum, the reciprocal 2^-27).
__device__ __forceinline__ int stratum_rel(const Strata& m, unsigned long long c0, unsigned long long d, double num0,
                                           double pow2F, double invS, long Kref, long ns) {
    const unsigned long long C = c0 + d;
    if (C >= m.total) return (int)(ns - Kref);
    const double y = ((double)d * pow2F + num0) * invS;
    long k = (long)(int)ceil(y);
    if (k < 0) k = 0;
    if (k > ns) k = ns;
    const unsigned long long B = C << m.F;
    const unsigned long long v = (unsigned long long)k * m.S + m.U;          // (t_k << F) + fractional bits
    if (v < B) { if (k < ns) ++k; }                                           // t_k < C: the next stratum is the first
    else if (k > 0 && v - m.S >= B) --k;                                      // t_{k-1} >= C already
    return (int)(k - Kref);
}

// The same for the items of ONE wave whose strata span T < 2^20: relative to the wave's first stratum K0 the quotient is
// small, so an fp32 estimate of ceil(X / S), X = Bw + (d << F) with the wave constant Bw = (c_start << F) - U - K0 S in
// (-S, 0], is off by less than one stratum and ONE exact 64-bit check decides (branch-free: 22 instead of ~45
// instructions + 3 divergent branches per item).  Same value as stratum_rel(..., Kref = K0) by construction.
__device__ __forceinline__ int stratum_rel_small(const Strata& m, long long Bw, float invS_f, unsigned long long C_abs,
                                                 unsigned long long d, int ns_rel) {
    const long long X = Bw + (long long)(d << m.F);
    const float xf = (float)(int)(X >> 32) * 4294967296.0f + (float)(unsigned)X;
    int k = (int)ceilf(xf * invS_f);
    k = k < 0 ? 0 : (k > ns_rel ? ns_rel : k);
    const long long R = X - (long long)((unsigned long long)(unsigned)k * m.S);        // X - k S, exact
    k += (R > 0 && k < ns_rel) ? 1 : 0;
    k -= (R + (long long)m.S <= 0 && k > 0) ? 1 : 0;
    return C_abs >= m.total ? ns_rel : k;
}

// Stratified resampling (include/fabhip.h: fabhip_resample_stratified; tests/resample_stratified_spec.py restates it): one
// hashed offset per stratum, t_k = (k S + U_k) >> F with U_k = hi64(ms_hash(seed, k) * S) in [0, S - 1].  The thresholds are
// still sorted, one per stratum, so the inverse stays a closed form: with B = C << F and q = min(floor(B / S), ns)
//     K(C) = #{k : t_k < C} = q + [q < ns and U_q < B - q S]
// (strata below q end at or below B, strata above q start above it; only stratum q needs its hash).  Both functions below take
// an ESTIMATE of q, make it exact with one integer step on the remainder R = B - q S, and let the hash of the exact q decide.

// K(c0 + d) - Kref as int32: float64 estimate of floor(((c0 + d) << F) / S) (B < 2^62, q <= ns + 1 < 2^31: the three rounded
// operations lose < 2^-20 of a stratum), B0d = (double)(c0 << F) supplied by the caller.
__device__ __forceinline__ int stratified_rel(const Strata& m, unsigned long long seed, unsigned long long c0,
                                              unsigned long long d, double B0d, double pow2F, double invS, long Kref, long ns) {
    const unsigned long long B = (c0 + d) << m.F;
    long long q = (long long)(((double)d * pow2F + B0d) * invS);
    long long R = (long long)(B - (unsigned long long)q * m.S);              // |R| < 2 S < 2^63
    if (R < 0) { --q; R += (long long)m.S; }
    else if (R >= (long long)m.S) { ++q; R -= (long long)m.S; }
    if (q >= ns) return (int)(ns - Kref);
    const unsigned long long Uq = __umul64hi(ms_hash(seed, (unsigned long long)q), m.S);
    return (int)(q + (Uq < (unsigned long long)R ? 1 : 0) - Kref);
}

// The same for the items of ONE wave whose strata span T < 2^20, relative to the stratum q0 = floor((c_start << F) / S) that
// holds the wave's start: X = Bw + (d << F) with the wave constant Bw = (c_start << F) - q0 S in [0, S), so the quotient
// floor(X / S) <= T + 1 is small and an fp32 estimate is off by less than one stratum (as in stratum_rel_small).  koff = K0 - q0
// (0 or 1) turns the count into one relative to the wave's first stratum K0.  Same value as stratified_rel(..., Kref = K0).
__device__ __forceinline__ int stratified_rel_small(const Strata& m, unsigned long long seed, unsigned long long Bw, float invS_f,
                                                    unsigned long long q0, unsigned long long d, int koff, long ns, int ns_rel) {
    const unsigned long long X = Bw + (d << m.F);
    const float xf = (float)(unsigned)(X >> 32) * 4294967296.0f + (float)(unsigned)X;
    int k = (int)(xf * invS_f);
    long long R = (long long)(X - (unsigned long long)(unsigned)k * m.S);    // X - k S, exact
    const bool lo = R < 0, hi = R >= (long long)m.S;
    k += hi ? 1 : (lo ? -1 : 0);
    R += lo ? (long long)m.S : (hi ? -(long long)m.S : 0ll);
    const unsigned long long q = q0 + (unsigned long long)(unsigned)k;
    const unsigned long long Uq = __umul64hi(ms_hash(seed, q), m.S);
    const int r = k + (Uq < (unsigned long long)R ? 1 : 0) - koff;
    return q >= (unsigned long long)ns ? ns_rel : r;
}

// The emitter of the systematic (STRAT = false) and of the stratified resampler (STRAT = true; `seed` is read by that one only):
// the two differ in the stratum ranges ke[] alone.
template <bool STRAT>
__device__ __forceinline__ void emit_runs(const float* __restrict__ lw, long n,
                                          const float* __restrict__ max_val,
                                          const unsigned long long* __restrict__ wave_sum,
                                          const unsigned long long* __restrict__ block_excl,
                                          const unsigned long long* __restrict__ strata_ptr,
                                          long ns, long long* __restrict__ idx,
                                          unsigned long long* __restrict__ giant_count,
                                          long long* __restrict__ giant_desc, long giant_cap, unsigned long long seed) {
    __shared__ __attribute__((aligned(16))) unsigned char em_lds[EM_NW * EM_WAVE_LDS];
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long wt = (long)blockIdx.x * EM_NW + wave;
    const long wbase = wt * EM_WAVE_ITEMS;
    if (wbase >= n) return;
    const Strata m = load_strata(strata_ptr);
    if (m.total == 0ull) {                                 // all weights zero: every stratum maps to the last index
        if (wt == 0)
            for (long k = lane; k < ns; k += 64) idx[k] = n - 1;
        return;
    }
    float* wf = reinterpret_cast<float*>(em_lds + (size_t)wave * EM_WAVE_LDS);
    int* win = reinterpret_cast<int*>(wf);
    const float mx = max_val[0];
    unsigned long long c_start = block_excl[blockIdx.x];
    for (int w = 0; w < wave; ++w) c_start += wave_sum[(long)blockIdx.x * EM_NW + w];
    // ---- CDF of this wave's 1024 weights: lane owns items [16 lane, 16 lane + 16) ----
    if (wbase + EM_WAVE_ITEMS <= n && (((size_t)lw & 15) == 0)) {
        float4 x[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) x[h] = *reinterpret_cast<const float4*>(lw + wbase + h * 256 + lane * 4);
#pragma unroll
        for (int h = 0; h < 4; ++h)                      // item 256 h + 4 lane -> row 16 h + lane / 4, column 4 (lane % 4)
            *reinterpret_cast<float4*>(wf + (16 * h + (lane >> 2)) * EM_FSTRIDE + 4 * (lane & 3)) = x[h];
    } else {
        for (int i = lane; i < EM_WAVE_ITEMS; i += 64)
            wf[(i >> 4) * EM_FSTRIDE + (i & 15)] = (wbase + i < n) ? lw[wbase + i] : -INFINITY;
    }
    __builtin_amdgcn_wave_barrier();
    unsigned long long run[16];
    unsigned long long acc = 0ull;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 y = *reinterpret_cast<const float4*>(wf + lane * EM_FSTRIDE + 4 * k);
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
    const unsigned long long wtot = shfl_u64(incl, 63);
    if (wtot == 0ull) return;                              // no stratum lands in a zero-weight tile
    const unsigned long long lane_off = incl - acc;        // CDF offset of this lane's first item inside the wave
    // ---- stratum ranges relative to K0 = K(c_start): item j owns [ke[j-1], ke[j]) (ke[-1] = previous lane's ke[15]) ----
    const double pow2F = (double)(1ull << m.F), invS = 1.0 / (double)m.S;
    const unsigned long long B0 = c_start << m.F;
    const double num0 = STRAT ? (double)B0 : (B0 >= m.U ? (double)(B0 - m.U) : -(double)(m.U - B0));
    const long K0 = STRAT ? (long)stratified_rel(m, seed, c_start, 0ull, num0, pow2F, invS, 0, ns)
                          : (long)stratum_rel(m, c_start, 0ull, num0, pow2F, invS, 0, ns);   // wave-uniform (Kref = 0: < 2^31)
    const int T = STRAT ? stratified_rel(m, seed, c_start, wtot, num0, pow2F, invS, K0, ns)
                        : stratum_rel(m, c_start, wtot, num0, pow2F, invS, K0, ns);          // strata owned by this wave (uniform)
    if (T <= 0) return;
    int ke[16];
    if constexpr (STRAT) {
        if (T < (1 << 20)) {                               // wave-uniform: the usual case
            const unsigned long long q0 = B0 / m.S;        // the stratum that holds c_start: K0 - q0 is 0 or 1 (T > 0: q0 < ns)
            const unsigned long long Bw = B0 - q0 * m.S;
            const float invS_f = 1.0f / (float)m.S;
            const int koff = (int)(K0 - (long)q0), ns_rel = (int)(ns - K0);
#pragma unroll
            for (int j = 0; j < 16; ++j)
                ke[j] = stratified_rel_small(m, seed, Bw, invS_f, q0, lane_off + run[j], koff, ns, ns_rel);
        } else {                                           // giant runs: float64 estimate per item
#pragma unroll
            for (int j = 0; j < 16; ++j)
                ke[j] = (j > 0 && run[j] == run[j - 1]) ? ke[j - 1]
                                                        : stratified_rel(m, seed, c_start, lane_off + run[j], num0, pow2F, invS, K0, ns);
        }
    } else if (T < (1 << 20)) {                            // wave-uniform: the usual case
        const long long Bw = (long long)(B0 - m.U - (unsigned long long)K0 * m.S);
        const float invS_f = 1.0f / (float)m.S;
        const int ns_rel = (int)(ns - K0);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            ke[j] = stratum_rel_small(m, Bw, invS_f, c_start + lane_off + run[j], lane_off + run[j], ns_rel);
    } else {                                               // giant runs: float64 estimate per item
#pragma unroll
        for (int j = 0; j < 16; ++j)
            ke[j] = (j > 0 && run[j] == run[j - 1]) ? ke[j - 1]
                                                    : stratum_rel(m, c_start, lane_off + run[j], num0, pow2F, invS, K0, ns);
    }
    int kprev = __shfl_up(ke[15], 1);
    if (lane == 0) kprev = 0;
    __builtin_amdgcn_wave_barrier();                       // every lane is done reading the float staging
    const long item0 = wbase;
    // giant runs: publish, the grid-wide fill kernel writes them; this wave skips windows entirely inside one
    unsigned gmask = 0u;                                   // bit j: item j of this lane is a PUBLISHED giant run
    if (T >= EM_GIANT) {                                   // wave-uniform
        int sg = kprev;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (ke[j] - sg >= EM_GIANT) {
                const unsigned long long slot = atomicAdd(giant_count, 1ull);
                // (list full: the run stays with this wave.  Reached through k_emit_systematic only: fabhip_resample_stratified
                //  carves its list for ns / EM_GIANT + 1 runs, more than can exist, so for STRAT this is a bound on the store
                //  below that never binds - kept as that, tested through the systematic cases list_full / no_list)
                if ((long)slot < giant_cap) {
                    long id = item0 + 16 * lane + j;
                    giant_desc[3 * slot] = K0 + sg; giant_desc[3 * slot + 1] = K0 + ke[j];
                    giant_desc[3 * slot + 2] = id < n ? id : n - 1;
                    gmask |= 1u << j;
                }
            }
            sg = ke[j];
        }
    }
    const bool wave_has_giant = __ballot(gmask != 0u) != 0ull;
    for (int w0 = 0; w0 < T; w0 += EM_WIN) {
        const int wlen = T - w0 < EM_WIN ? T - w0 : EM_WIN;
        const int whi = w0 + wlen;
        if (wave_has_giant) {                              // a window entirely inside ONE published giant run: skip
            bool cover = false;
            int sg = kprev;
#pragma unroll
            for (int j = 0; j < 16; ++j) { if (((gmask >> j) & 1u) && sg <= w0 && ke[j] >= whi) cover = true; sg = ke[j]; }
            if (__ballot(cover) != 0ull) continue;
        }
        // (a) clear the window, (b) every non-empty run drops its id + 1 at max(run start, window start)
#pragma unroll
        for (int i = 0; i < 64 * EM_WSTRIDE / 256; ++i)
            *reinterpret_cast<int4*>(win + 4 * lane + 256 * i) = make_int4(0, 0, 0, 0);
        __builtin_amdgcn_wave_barrier();
        {
            int sg = kprev;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int e = ke[j];
                const int pos = sg > w0 ? sg : w0;
                if (e > pos && pos < whi) win[em_waddr(pos - w0)] = 16 * lane + j + 1;
                sg = e;
            }
        }
        __builtin_amdgcn_wave_barrier();
        // (c) inclusive max-scan: lane owns entries [32 lane, 32 lane + 32)
        int v[EM_ROW];
#pragma unroll
        for (int i = 0; i < EM_ROW / 4; ++i) {
            const int4 q = *reinterpret_cast<const int4*>(win + EM_WSTRIDE * lane + 4 * i);
            v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
        }
#pragma unroll
        for (int i = 1; i < EM_ROW; ++i) v[i] = v[i] > v[i - 1] ? v[i] : v[i - 1];
        int mx_in = v[EM_ROW - 1];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(mx_in, off);
            if (lane >= off) mx_in = mx_in > o ? mx_in : o;
        }
        int carry = __shfl_up(mx_in, 1);
        if (lane == 0) carry = 0;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < EM_ROW / 4; ++i) {
            int4 q;
            q.x = (v[4 * i] > carry ? v[4 * i] : carry) - 1;
            q.y = (v[4 * i + 1] > carry ? v[4 * i + 1] : carry) - 1;
            q.z = (v[4 * i + 2] > carry ? v[4 * i + 2] : carry) - 1;
            q.w = (v[4 * i + 3] > carry ? v[4 * i + 3] : carry) - 1;
            *reinterpret_cast<int4*>(win + EM_WSTRIDE * lane + 4 * i) = q;
        }
        __builtin_amdgcn_wave_barrier();
        // (d) flush: 4 entries per lane per step -> two 16-byte stores
        const long obase = K0 + w0;
        for (int p = 4 * lane; p < wlen; p += 256) {
            const int4 q = *reinterpret_cast<const int4*>(win + em_waddr(p));
            long r0 = item0 + q.x, r1 = item0 + q.y, r2 = item0 + q.z, r3 = item0 + q.w;
            if (r3 >= n) { r0 = r0 < n ? r0 : n - 1; r1 = r1 < n ? r1 : n - 1; r2 = r2 < n ? r2 : n - 1; r3 = n - 1; }
            if (p + 4 <= wlen) {
                i64x2* o = reinterpret_cast<i64x2*>(idx + obase + p);
                o[0] = (i64x2){r0, r1};
                o[1] = (i64x2){r2, r3};
            } else {
                idx[obase + p] = r0;
                if (p + 1 < wlen) idx[obase + p + 1] = r1;
                if (p + 2 < wlen) idx[obase + p + 2] = r2;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__global__ __launch_bounds__(64 * EM_NW) void k_emit_systematic(const float* __restrict__ lw, long n,
                                                                const float* __restrict__ max_val,
                                                                const unsigned long long* __restrict__ wave_sum,
                                                                const unsigned long long* __restrict__ block_excl,
                                                                const unsigned long long* __restrict__ strata_ptr,
                                                                long ns, long long* __restrict__ idx,
                                                                unsigned long long* __restrict__ giant_count,
                                                                long long* __restrict__ giant_desc, long giant_cap) {
    emit_runs<false>(lw, n, max_val, wave_sum, block_excl, strata_ptr, ns, idx, giant_count, giant_desc, giant_cap, 0ull);
}

// (strata_ptr: k_emit_prefix with u0 = 0, i.e. {total, S, 0, F})
__global__ __launch_bounds__(64 * EM_NW) void k_emit_stratified(const float* __restrict__ lw, long n,
                                                                const float* __restrict__ max_val,
                                                                const unsigned long long* __restrict__ wave_sum,
                                                                const unsigned long long* __restrict__ block_excl,
                                                                const unsigned long long* __restrict__ strata_ptr,
                                                                long ns, unsigned long long seed, long long* __restrict__ idx,
                                                                unsigned long long* __restrict__ giant_count,
                                                                long long* __restrict__ giant_desc, long giant_cap) {
    emit_runs<true>(lw, n, max_val, wave_sum, block_excl, strata_ptr, ns, idx, giant_count, giant_desc, giant_cap, seed);
}

// constant fill of the published giant runs: workgroup b takes 16384-entry chunks (run r, chunk c) round-robin
__global__ __launch_bounds__(256) void k_emit_fill_runs(const unsigned long long* __restrict__ giant_count,
                                                        const long long* __restrict__ giant_desc, long giant_cap,
                                                        long long* __restrict__ idx) {
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    long cnt = (long)*giant_count;
    if (cnt > giant_cap) cnt = giant_cap;
    constexpr long CH = 16384;
    unsigned work = 0;
    for (long r = 0; r < cnt; ++r) {
        const long a = giant_desc[3 * r], b = giant_desc[3 * r + 1], id = giant_desc[3 * r + 2];
        const long nch = (b - a + CH - 1) / CH;
        for (long c = 0; c < nch; ++c, ++work) {
            if (work % gridDim.x != blockIdx.x) continue;
            const long lo = a + c * CH, hi = lo + CH < b ? lo + CH : b;
            long p = lo + 2 * threadIdx.x;
            if ((lo & 1) && threadIdx.x == 0) idx[lo] = id;           // align the 16-byte stores
            p += (lo & 1);
            for (; p + 1 < hi; p += 512) *reinterpret_cast<i64x2*>(idx + p) = (i64x2){id, id};
            if (p < hi) idx[p] = id;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Seeded streaming multinomial resampling (include/fabhip.h: fabhip_resample_multinomial_stream; tests/resample_stream_spec.py
// restates it op for op).  The sorted values of ns iid uniforms are U_(k) = G_k / G_ns, G_k = e_0 + .. + e_k, with ns + 1
// exponential spacings e_i = fixed-point -ln(u_i), u_i a pure function of (seed, i): no noise tensor, any wave regenerates the
// spacings it needs in registers.  Sorted thresholds turn resampling into a MERGE of the draws with the CDF:
//     draw k selects the first j with C_j G_ns > G_k total, i.e. weight j owns the draws [K(C_{j-1}), K(C_j)),
//     K(C) = #{k < ns : G_k total < C G_ns}                                   (128-bit products, exact)
//   k_emit_wave_sums / k_emit_prefix  (the systematic resampler's)  tile sums of W and their prefix, total
//   k_ms_spacing_sums / k_emit_prefix / k_ms_tile_prefix            tile sums of e, inclusive prefix of every 1024-spacing tile
//   k_ms_bounds   one wave per 1024-weight tile: K(c_start) - a 64-ary search of the spacing-tile prefixes, then an exact count
//                 inside ONE regenerated tile
//   k_ms_emit     the wave re-derives the CDF of its 1024 weights into LDS (as k_emit_systematic does), walks the spacing tiles
//                 its draws [K0, K1) touch, regenerates each tile's G_k (16 consecutive per lane + one wave scan), turns G_k into
//                 the integer threshold floor(G_k total / G_ns) - c_start (float64 estimate + one exact correction on the
//                 wrapped 64-bit remainder) and bisects the LDS CDF; the indices leave through an LDS transpose as 32-byte
//                 per-lane coalesced stores.  Weights that own >= 8192 draws are located exactly (two more K() evaluations),
//                 published and filled grid-wide by k_emit_fill_runs; the wave jumps over the spacing tiles inside such a run.
//   k_ms_shuffle  order = shuffled: out[k] = idx[pi(k)], pi the Feistel / cycle-walking bijection of k_random_order keyed by the seed
// ------------------------------------------------------------------------------------------------
constexpr long long MS_LN2_FIX = 186065279;             // round(ln 2 * 2^28)
constexpr unsigned long long MS_KEY_BASE = 1ull << 40;  // counters of the permutation's round keys (beyond every spacing index)
constexpr int MS_TILE = 1024;                           // spacings per tile (one wave: 16 consecutive per lane)
constexpr int MS_CDF_LDS = (1024 + 64) * 8;             // the wave's relative CDF, rows of 16 + 1 pad (aliases the float staging)
constexpr int MS_ITEM_LDS = (1024 + 64) * 4;            // the tile's selected items, rows of 16 + 1 pad
constexpr int MS_GMAX = 32;                             // published giant runs remembered per wave
constexpr int MS_WAVE_LDS = MS_CDF_LDS + MS_ITEM_LDS + 2 * MS_GMAX * 8;
constexpr long MS_GIANT_MIN = 8192;                     // runs at least this long are published
constexpr double MS_GIANT_EST = 16384.0;                // ... when the weight's EXPECTED run is at least this long
static_assert(MS_CDF_LDS >= 64 * EM_FSTRIDE * 4, "float staging must fit under the CDF");

__device__ __forceinline__ unsigned ms_mix32(unsigned x) {              // (murmur3 finaliser, topk.hip: tk_mix)
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

// e_i: fixed-point (28 fractional bits) -ln of u = f 2^-(lz + 1), f the top 24 bits of the odd 32-bit word y as a float in
// [1, 2).  Integer operations and individually rounded float32 multiplies / adds only (no contraction in this file).
__device__ __forceinline__ unsigned long long ms_spacing(unsigned long long seed, unsigned long long i) {
    const unsigned y = (unsigned)(ms_hash(seed, i) >> 32) | 1u;
    const int lz = __clz((int)y);
    const unsigned mant = (y << lz) >> 8;
    const float f = (float)mant * 1.1920928955078125e-07f;            // exact
    const bool red = f >= 1.41421354f;
    const float g = red ? f * 0.5f : f;
    const float t = g - 1.0f;                                         // exact
    float p = 0.08743945509195328f;
    p = p * t + -0.14377330243587494f;
    p = p * t + 0.14949095249176025f;
    p = p * t + -0.16560696065425873f;
    p = p * t + 0.19956977665424347f;
    p = p * t + -0.2500215470790863f;
    p = p * t + 0.3333418369293213f;
    p = p * t + -0.49999988079071045f;
    p = p * t + 1.0f;
    p = p * t;
    const long long e = (long long)(lz + 1 - (red ? 1 : 0)) * MS_LN2_FIX - (long long)(int)rintf(p * 268435456.0f);
    return e < 1 ? 1ull : (unsigned long long)e;
}

struct U128 { unsigned long long hi, lo; };
__device__ __forceinline__ U128 mul128(unsigned long long a, unsigned long long b) { return U128{__umul64hi(a, b), a * b}; }
__device__ __forceinline__ bool lt128(const U128& a, const U128& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ int ms_pad(int p) { return p + (p >> 4); }

__global__ __launch_bounds__(64 * EM_NW) void k_ms_spacing_sums(unsigned long long seed, long ns,
                                                                unsigned long long* __restrict__ wave_sum,
                                                                unsigned long long* __restrict__ block_sum) {
    __shared__ unsigned long long wsum[EM_NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long wt = (long)blockIdx.x * EM_NW + wave;
    const long base = wt * MS_TILE;
    unsigned long long acc = 0ull;
#pragma unroll 4
    for (int j = 0; j < MS_TILE / 64; ++j) {
        const long i = base + 64 * j + lane;
        if (i <= ns) acc += ms_spacing(seed, (unsigned long long)i);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += shfl_u64(acc, lane ^ off);
    if (lane == 0) { wsum[wave] = acc; if (base <= ns) wave_sum[wt] = acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = 0ull;
        for (int w = 0; w < EM_NW; ++w) b += wsum[w];
        block_sum[blockIdx.x] = b;
    }
}

// inclusive prefix at the end of every spacing tile: tinc[t] = G_{min(1024 t + 1023, ns)}
__global__ __launch_bounds__(256) void k_ms_tile_prefix(const unsigned long long* __restrict__ wave_sum,
                                                        const unsigned long long* __restrict__ block_excl, long nt,
                                                        unsigned long long* __restrict__ tinc) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    unsigned long long s = block_excl[t / EM_NW];
    for (long w = t / EM_NW * EM_NW; w <= t; ++w) s += wave_sum[w];
    tinc[t] = s;
}

// G_k of the spacings of tile t, 16 consecutive per lane: g[j] = G_{1024 t + 16 lane + j} (indices beyond ns repeat G_ns)
__device__ __forceinline__ void ms_tile_sums(unsigned long long seed, long ns, long t, const unsigned long long* __restrict__ tinc,
                                             int lane, unsigned long long (&g)[16]) {
    const long i0 = t * MS_TILE + 16 * lane;
    unsigned long long acc = 0ull;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (i0 + j <= ns) acc += ms_spacing(seed, (unsigned long long)(i0 + j));
        g[j] = acc;
    }
    unsigned long long incl = acc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = shfl_up_u64(incl, off);
        if (lane >= off) incl += o;
    }
    const unsigned long long off0 = incl - acc + (t > 0 ? tinc[t - 1] : 0ull);
#pragma unroll
    for (int j = 0; j < 16; ++j) g[j] += off0;
}

// K(C) = #{k < ns : G_k total < C G_ns}, C wave-uniform, the whole wave calls it.  64-ary search for the first spacing tile
// whose last G reaches C (the last tile always does: G_ns total >= C G_ns), then the exact count inside that tile.
__device__ __forceinline__ long ms_count_below(unsigned long long C, unsigned long long total, unsigned long long Gn,
                                               unsigned long long seed, long ns, const unsigned long long* __restrict__ tinc,
                                               long nte, int lane) {
    if (C == 0ull) return 0;
    if (C >= total) return ns;
    const U128 rhs = mul128(C, Gn);
    long lo = 0, hi = nte;
    while (hi - lo > 1) {
        const long step = (hi - lo + 63) >> 6;
        long i = lo + (long)(lane + 1) * step - 1;
        if (i > hi - 1) i = hi - 1;
        const bool reached = !lt128(mul128(tinc[i], total), rhs);
        const unsigned long long m = __ballot(reached);
        if (m == 0ull) return ns;                          // (cannot happen: lane 63 probes hi - 1)
        const int f = __ffsll((long long)m) - 1;
        lo += (long)f * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    unsigned long long g[16];
    ms_tile_sums(seed, ns, lo, tinc, lane, g);
    const long i0 = lo * MS_TILE + 16 * lane;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) cnt += (i0 + j < ns && lt128(mul128(g[j], total), rhs)) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    return lo * MS_TILE + cnt;
}

// kb[w] = K(c_start of weight tile w), w = 0 .. nwt (kb[nwt] = ns); nothing when every weight is zero
__global__ __launch_bounds__(64 * EM_NW) void k_ms_bounds(const unsigned long long* __restrict__ wave_sum,
                                                          const unsigned long long* __restrict__ block_excl, long nwt,
                                                          const unsigned long long* __restrict__ strata_w,
                                                          const unsigned long long* __restrict__ strata_e,
                                                          unsigned long long seed, long ns,
                                                          const unsigned long long* __restrict__ tinc, long nte,
                                                          long long* __restrict__ kb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long w = (long)blockIdx.x * EM_NW + wave;
    const unsigned long long total = strata_w[0], Gn = strata_e[0];
    if (w > nwt || total == 0ull) return;
    long k = ns;
    if (w < nwt) {
        unsigned long long c = block_excl[w / EM_NW];
        for (long v = w / EM_NW * EM_NW; v < w; ++v) c += wave_sum[v];
        k = ms_count_below(c, total, Gn, seed, ns, tinc, nte, lane);
    }
    if (lane == 0) kb[w] = k;
}

__global__ __launch_bounds__(64 * EM_NW) void k_ms_emit(const float* __restrict__ lw, long n, const float* __restrict__ max_val,
                                                        const unsigned long long* __restrict__ wave_sum,
                                                        const unsigned long long* __restrict__ block_excl,
                                                        const unsigned long long* __restrict__ strata_w,
                                                        const unsigned long long* __restrict__ strata_e,
                                                        unsigned long long seed, long ns,
                                                        const unsigned long long* __restrict__ tinc, long nte,
                                                        const long long* __restrict__ kb, long long* __restrict__ idx,
                                                        unsigned long long* __restrict__ giant_count,
                                                        long long* __restrict__ giant_desc, long giant_cap) {
    __shared__ __attribute__((aligned(16))) unsigned char ms_lds[EM_NW * MS_WAVE_LDS];
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long wt = (long)blockIdx.x * EM_NW + wave;
    const long wbase = wt * EM_WAVE_ITEMS;
    if (wbase >= n) return;
    const unsigned long long total = strata_w[0];
    if (total == 0ull) {                                   // all weights zero: every draw maps to the last index
        if (wt == 0)
            for (long k = lane; k < ns; k += 64) idx[k] = n - 1;
        return;
    }
    const long K0 = kb[wt], K1 = kb[wt + 1];               // this wave's draws (wave-uniform)
    if (K1 <= K0) return;
    const unsigned long long Gn = strata_e[0];
    unsigned char* wl = ms_lds + (size_t)wave * MS_WAVE_LDS;
    float* wf = reinterpret_cast<float*>(wl);
    unsigned long long* crel = reinterpret_cast<unsigned long long*>(wl);
    int* itm = reinterpret_cast<int*>(wl + MS_CDF_LDS);
    long long* ga = reinterpret_cast<long long*>(wl + MS_CDF_LDS + MS_ITEM_LDS);
    long long* gb = ga + MS_GMAX;
    const float mx = max_val[0];
    unsigned long long c_start = block_excl[blockIdx.x];
    for (int w = 0; w < wave; ++w) c_start += wave_sum[(long)blockIdx.x * EM_NW + w];
    // ---- CDF of this wave's 1024 weights relative to c_start: lane owns items [16 lane, 16 lane + 16) (k_emit_systematic) ----
    if (wbase + EM_WAVE_ITEMS <= n && (((size_t)lw & 15) == 0)) {
        float4 x[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) x[h] = *reinterpret_cast<const float4*>(lw + wbase + h * 256 + lane * 4);
#pragma unroll
        for (int h = 0; h < 4; ++h)
            *reinterpret_cast<float4*>(wf + (16 * h + (lane >> 2)) * EM_FSTRIDE + 4 * (lane & 3)) = x[h];
    } else {
        for (int i = lane; i < EM_WAVE_ITEMS; i += 64)
            wf[(i >> 4) * EM_FSTRIDE + (i & 15)] = (wbase + i < n) ? lw[wbase + i] : -INFINITY;
    }
    __builtin_amdgcn_wave_barrier();
    unsigned long long run[16];
    unsigned long long acc = 0ull;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 y = *reinterpret_cast<const float4*>(wf + lane * EM_FSTRIDE + 4 * k);
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
    const unsigned long long lane_off = incl - acc;
    // weights whose EXPECTED run is long: candidates for the grid-wide fill (decided exactly below)
    unsigned cand = 0u;
    if (K1 - K0 >= MS_GIANT_MIN) {                         // wave-uniform
        const double scale = (double)ns / (double)total;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned long long wj = run[j] - (j ? run[j - 1] : 0ull);
            if ((double)wj * scale >= MS_GIANT_EST) cand |= 1u << j;
        }
    }
    __builtin_amdgcn_wave_barrier();                       // every lane is done reading the float staging
#pragma unroll
    for (int j = 0; j < 16; ++j) crel[17 * lane + j] = lane_off + run[j];
    __builtin_amdgcn_wave_barrier();
    int gcnt = 0;                                          // published runs of this wave (wave-uniform)
    while (gcnt < MS_GMAX) {
        const unsigned long long m = __ballot(cand != 0u);
        if (m == 0ull) break;
        const int src = __ffsll((long long)m) - 1;
        const unsigned cm = (unsigned)__shfl((int)cand, src);
        const int j = __ffs((int)cm) - 1;
        if (lane == src) cand &= cand - 1u;
        const int pos = 16 * src + j;
        const unsigned long long cj = crel[ms_pad(pos)], cp = pos ? crel[ms_pad(pos - 1)] : 0ull;
        const long a = ms_count_below(c_start + cp, total, Gn, seed, ns, tinc, nte, lane);
        const long b = ms_count_below(c_start + cj, total, Gn, seed, ns, tinc, nte, lane);
        if (b - a < MS_GIANT_MIN) continue;
        unsigned long long slot = 0ull;
        if (lane == 0) slot = atomicAdd(giant_count, 1ull);
        slot = shfl_u64(slot, 0);
        if ((long)slot >= giant_cap) break;                // (list full: the run stays with this wave)
        if (lane == 0) {
            const long id = wbase + pos;
            giant_desc[3 * slot] = a; giant_desc[3 * slot + 1] = b; giant_desc[3 * slot + 2] = id < n ? id : n - 1;
            ga[gcnt] = a; gb[gcnt] = b;
        }
        ++gcnt;
    }
    __builtin_amdgcn_wave_barrier();
    // ---- the spacing tiles this wave's draws touch ----
    const U128 Bc = mul128(c_start, Gn);
    const double invGn = 1.0 / (double)Gn;
    const long t_last = (K1 - 1) / MS_TILE;
    for (long t = K0 / MS_TILE; t <= t_last;) {
        if (gcnt > 0) {                                    // draws of this tile all inside ONE published run: jump to its end
            const long dlo = K0 > t * MS_TILE ? K0 : t * MS_TILE, dhi = K1 < (t + 1) * MS_TILE ? K1 : (t + 1) * MS_TILE;
            const long long ra = lane < gcnt ? ga[lane] : 0, rb = lane < gcnt ? gb[lane] : 0;
            const unsigned long long m = __ballot(lane < gcnt && ra <= dlo && rb >= dhi);
            if (m != 0ull) {
                const long e = shfl_i64(rb, __ffsll((long long)m) - 1);
                if (e >= K1) break;
                t = e / MS_TILE;
                continue;
            }
        }
        unsigned long long g[16];
        ms_tile_sums(seed, ns, t, tinc, lane, g);
        const long k0 = t * MS_TILE + 16 * lane;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long k = k0 + j;
            const bool inr = k >= K0 && k < K1;
            // q = floor(G_k total / G_ns) - c_start = floor((G_k total - c_start G_ns) / G_ns) in [0, wave total)
            const U128 A = mul128(g[j], total);
            const unsigned long long rlo = A.lo - Bc.lo, rhi = A.hi - Bc.hi - (A.lo < Bc.lo ? 1ull : 0ull);
            const double est = inr ? ((double)rhi * 18446744073709551616.0 + (double)rlo) * invGn : 0.0;
            unsigned long long q = (unsigned long long)est;                     // off by at most one
            const long long rem = (long long)(rlo - q * Gn);                   // |R - q G_ns| < 2 G_ns < 2^63: the wrap is exact
            if (rem < 0) --q;
            else if (rem >= (long long)Gn) ++q;
            if (!inr) q = 0ull;
            int pos = 0;                                   // entries <= q  =  first entry > q
#pragma unroll
            for (int s = 512; s > 0; s >>= 1) {
                const int p = pos + s - 1;
                if (crel[ms_pad(p)] <= q) pos += s;
            }
            itm[17 * lane + j] = pos < 1023 ? pos : 1023;
        }
        __builtin_amdgcn_wave_barrier();
        for (int p = 4 * lane; p < MS_TILE; p += 256) {
            const long k = t * MS_TILE + p;
            const int b0 = ms_pad(p);
            long r0 = wbase + itm[b0], r1 = wbase + itm[b0 + 1], r2 = wbase + itm[b0 + 2], r3 = wbase + itm[b0 + 3];
            r0 = r0 < n ? r0 : n - 1; r1 = r1 < n ? r1 : n - 1; r2 = r2 < n ? r2 : n - 1; r3 = r3 < n ? r3 : n - 1;
            if (k >= K0 && k + 3 < K1) {
                i64x2* o = reinterpret_cast<i64x2*>(idx + k);
                o[0] = (i64x2){r0, r1};
                o[1] = (i64x2){r2, r3};
            } else {
                if (k >= K0 && k < K1) idx[k] = r0;
                if (k + 1 >= K0 && k + 1 < K1) idx[k + 1] = r1;
                if (k + 2 >= K0 && k + 2 < K1) idx[k + 2] = r2;
                if (k + 3 >= K0 && k + 3 < K1) idx[k + 3] = r3;
            }
        }
        __builtin_amdgcn_wave_barrier();
        ++t;
    }
}

__global__ __launch_bounds__(256) void k_ms_shuffle(const long long* __restrict__ idx_in, long ns, unsigned long long seed,
                                                    long long* __restrict__ idx_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    int bits = 2;
    while ((1l << bits) < ns) ++bits;
    const int lb = bits >> 1, rb = bits - lb;
    const unsigned lm = (1u << lb) - 1u, rm = (1u << rb) - 1u;
    unsigned key[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) key[j] = (unsigned)ms_hash(seed, MS_KEY_BASE + (unsigned long long)j);
    unsigned long v = (unsigned long)i;
    do {
        unsigned l = (unsigned)(v >> rb) & lm, r = (unsigned)v & rm;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j & 1) r ^= ms_mix32(l ^ key[j]) & rm;
            else l ^= ms_mix32(r ^ key[j]) & lm;
        }
        v = ((unsigned long)l << rb) | r;
    } while ((long)v >= ns);
    idx_out[i] = idx_in[v];
}

// ------------------------------------------------------------------------------------------------
// Host path of the emit family.  Every entry point: validate, carve, emit_front (maximum, tile sums, block prefix + stratum
// map), its own emit kernel, emit_finish (grid-wide fill of the published giant runs, the shuffle of order = shuffled).
// ------------------------------------------------------------------------------------------------
struct EmitWs {           // what the kernels the three resamplers share read and write
    float *max_part, *max_val;                                     // [1024], [1]
    unsigned long long *wave_sum, *block_sum, *block_excl;         // [nwt] tile sums, [nbk] block sums, their exclusive prefix
    unsigned long long* strata;                                    // {total, S, U, F}; the giant-run counter is strata + 4
    long long* giant_desc;                                         // [3 giant_cap]
    long giant_cap, nwt, nbk;
};

// The common blocks, out of `b` (launch.h: Bump).  max_part / max_val: where the caller has them already (null: carved here).  giant_min: the
// shortest run that is published - at most ns / giant_min + 1 can exist.  room: the 8-byte words the blocks may take in all
// (< 0: no limit): what the fixed blocks, nwt + 2 nbk + 5 words, leave of it bounds the list of runs, 3 words each.
static EmitWs carve_emit_ws(Bump& b, float* max_part, float* max_val, long n, long ns, long giant_min, long room) {
    EmitWs w;
    w.nwt = (n + EM_WAVE_ITEMS - 1) / EM_WAVE_ITEMS; w.nbk = (n + EM_BLOCK - 1) / EM_BLOCK;
    w.giant_cap = ns / giant_min + 1;
    if (room >= 0) {
        long left = (room - (w.nwt + 2 * w.nbk + 5)) / 3;
        if (left < 0) left = 0;
        if (w.giant_cap > left) w.giant_cap = left;
    }
    w.max_part = max_part ? max_part : b.take<float>(1024);
    w.max_val = max_val ? max_val : b.take<float>(1);
    w.wave_sum = b.take<unsigned long long>((size_t)w.nwt);
    w.block_sum = b.take<unsigned long long>((size_t)w.nbk);
    w.block_excl = b.take<unsigned long long>((size_t)w.nbk);
    w.strata = b.take<unsigned long long>(5);
    w.giant_desc = b.take<long long>((size_t)w.giant_cap * 3);
    return w;
}

static void emit_front(const float* log_w, long n, const EmitWs& w, double u0, long ns, hipStream_t st) {
    launch_max(log_w, n, w.max_part, w.max_val, st);
    hipLaunchKernelGGL(k_emit_wave_sums, dim3((unsigned)w.nbk), dim3(64 * EM_NW), 0, st, log_w, n, w.max_val, w.wave_sum,
                       w.block_sum);
    hipLaunchKernelGGL(k_emit_prefix, dim3(1), dim3(1024), 0, st, w.block_sum, w.nbk, w.block_excl, u0, ns, w.strata, w.strata + 4);
}

// out: where the emit kernel wrote (idx itself, or the `sorted` block when order = shuffled)
static int emit_finish(const EmitWs& w, long long* out, long long* idx, long ns, long giant_min, int order,
                       unsigned long long seed, hipStream_t st) {
    if (w.giant_cap > 0 && ns >= giant_min)
        hipLaunchKernelGGL(k_emit_fill_runs, dim3(256), dim3(256), 0, st, w.strata + 4, w.giant_desc, w.giant_cap, out);
    if (order == FABHIP_ORDER_SHUFFLED)
        hipLaunchKernelGGL(k_ms_shuffle, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, out, ns, seed, idx);
    return check_launch();
}

struct StratWs {          // workspace layout of the stratified resampler (all 256-byte aligned)
    EmitWs w;                                                      // strata: {total, S, 0, F}
    long long* sorted;                                             // [n_samples] the sorted indices of order = shuffled
    size_t bytes;
};
static StratWs carve_strat_ws(void* workspace, long n, long ns) {
    StratWs s;
    Bump b{(char*)workspace, 256};
    s.w = carve_emit_ws(b, nullptr, nullptr, n, ns, EM_GIANT, -1);
    s.sorted = b.take<long long>((size_t)ns);
    s.bytes = (size_t)(b.p - (char*)workspace);
    return s;
}

struct StreamWs {         // workspace layout of the streaming multinomial resampler (all 256-byte aligned)
    EmitWs w;                                                      // the weights' side
    unsigned long long *e_wave, *e_block, *e_excl, *e_strata;      // spacings: tile sums, block sums, prefix, {total, ..}
    unsigned long long* tinc;                                      // [nte] inclusive prefix at the end of every spacing tile
    long long* kb;                                                 // [nwt + 1] first draw of every weight tile
    long long* sorted;                                             // [n_samples] the sorted indices of order = shuffled
    long nte, nbe;
    size_t bytes;
};
static StreamWs carve_stream_ws(void* workspace, long n, long ns) {
    StreamWs s;
    Bump b{(char*)workspace, 256};
    s.w = carve_emit_ws(b, nullptr, nullptr, n, ns, MS_GIANT_MIN, -1);
    s.nte = ns / MS_TILE + 1;                                      // spacings 0 .. ns
    s.nbe = (s.nte + EM_NW - 1) / EM_NW;
    s.e_wave = b.take<unsigned long long>((size_t)s.nbe * EM_NW);
    s.e_block = b.take<unsigned long long>((size_t)s.nbe);
    s.e_excl = b.take<unsigned long long>((size_t)s.nbe);
    s.e_strata = b.take<unsigned long long>(5);
    s.tinc = b.take<unsigned long long>((size_t)s.nte);
    s.kb = b.take<long long>((size_t)s.w.nwt + 1);
    s.sorted = b.take<long long>((size_t)ns);
    s.bytes = (size_t)(b.p - (char*)workspace);
    return s;
}

}  // namespace fab

using namespace fab;

extern "C" {

int fabhip_resample_systematic(const float* log_w, int64_t n, double u0, int64_t n_samples, int64_t* idx,
                               void* workspace, size_t workspace_bytes, fabhip_stream_t stream) {
    if (!log_w || !idx || !workspace || n < 1 || n_samples < 0 || !(u0 >= 0.0 && u0 < 1.0)) return FABHIP_EINVAL;
    if (((size_t)workspace & 255) != 0) return FABHIP_EINVAL;
    if (workspace_bytes < fabhip_resample_workspace_bytes(n)) return FABHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    if (n_samples == 0) return FABHIP_OK;
    const long ns = (long)n_samples;
    // FABHIP_OPT_SYSTEMATIC_VARIANT 0 = scan + CDF in HBM + search (A/B reference)
    if (option(FABHIP_OPT_SYSTEMATIC_VARIANT) == 0 || n_samples >= (1ll << 31) - 2)
        return systematic_by_search(log_w, (long)n, u0, ns, (long long*)idx, workspace, st);
    // fused path: no CDF in HBM; the scratch lives in the (8 n)-byte `cdf` region of the workspace, packed in 8-byte words -
    // the list of giant runs gets what is left of the region
    float *max_part, *max_val;
    unsigned long long* cdf;
    scan_ws_regions(workspace, (long)n, &max_part, &max_val, &cdf);
    Bump b{(char*)cdf, 8};
    const EmitWs w = carve_emit_ws(b, max_part, max_val, (long)n, ns, EM_GIANT, (long)n);
    emit_front(log_w, (long)n, w, u0, ns, st);
    hipLaunchKernelGGL(k_emit_systematic, dim3((unsigned)w.nbk), dim3(64 * EM_NW), 0, st, log_w, (long)n, w.max_val, w.wave_sum,
                       w.block_excl, w.strata, ns, (long long*)idx, w.strata + 4, w.giant_desc, w.giant_cap);
    return emit_finish(w, (long long*)idx, (long long*)idx, ns, EM_GIANT, FABHIP_ORDER_SORTED, 0ull, st);
}

size_t fabhip_resample_stream_workspace_bytes(int64_t n, int64_t n_samples) {
    if (n < 1 || n_samples < 1 || n_samples > FABHIP_STREAM_MAX_SAMPLES) return 0;
    return carve_stream_ws(nullptr, (long)n, (long)n_samples).bytes;
}

int fabhip_resample_multinomial_stream(const float* log_w, int64_t n, uint64_t seed, int64_t n_samples, int32_t order,
                                       int64_t* idx, void* workspace, size_t workspace_bytes, fabhip_stream_t stream) {
    if (!log_w || !idx || !workspace || n < 1 || n_samples < 1) return FABHIP_EINVAL;
    if (order != FABHIP_ORDER_SORTED && order != FABHIP_ORDER_SHUFFLED) return FABHIP_EINVAL;
    if (n_samples > FABHIP_STREAM_MAX_SAMPLES) return FABHIP_EINVAL;
    if (((size_t)workspace & 255) != 0) return FABHIP_EINVAL;
    if (workspace_bytes < fabhip_resample_stream_workspace_bytes(n, n_samples)) return FABHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    const long ns = (long)n_samples;
    const StreamWs s = carve_stream_ws(workspace, (long)n, ns);
    const EmitWs& w = s.w;
    long long* out = order == FABHIP_ORDER_SHUFFLED ? s.sorted : (long long*)idx;
    emit_front(log_w, (long)n, w, 0.0, ns, st);
    const dim3 block(64 * EM_NW);
    hipLaunchKernelGGL(k_ms_spacing_sums, dim3((unsigned)s.nbe), block, 0, st, (unsigned long long)seed, ns, s.e_wave, s.e_block);
    hipLaunchKernelGGL(k_emit_prefix, dim3(1), dim3(1024), 0, st, s.e_block, s.nbe, s.e_excl, 0.0, ns, s.e_strata, s.e_strata + 4);
    hipLaunchKernelGGL(k_ms_tile_prefix, dim3((unsigned)((s.nte + 255) / 256)), dim3(256), 0, st, s.e_wave, s.e_excl, s.nte, s.tinc);
    hipLaunchKernelGGL(k_ms_bounds, dim3((unsigned)((w.nwt + 1 + EM_NW - 1) / EM_NW)), block, 0, st, w.wave_sum, w.block_excl, w.nwt,
                       w.strata, s.e_strata, (unsigned long long)seed, ns, s.tinc, s.nte, s.kb);
    hipLaunchKernelGGL(k_ms_emit, dim3((unsigned)w.nbk), block, 0, st, log_w, (long)n, w.max_val, w.wave_sum, w.block_excl, w.strata,
                       s.e_strata, (unsigned long long)seed, ns, s.tinc, s.nte, s.kb, out, w.strata + 4, w.giant_desc, w.giant_cap);
    return emit_finish(w, out, (long long*)idx, ns, MS_GIANT_MIN, order, (unsigned long long)seed, st);
}

size_t fabhip_resample_stratified_workspace_bytes(int64_t n, int64_t n_samples) {
    if (n < 1 || n_samples < 1 || n_samples > FABHIP_STRATIFIED_MAX_SAMPLES) return 0;
    return carve_strat_ws(nullptr, (long)n, (long)n_samples).bytes;
}

int fabhip_resample_stratified(const float* log_w, int64_t n, uint64_t seed, int64_t n_samples, int32_t order, int64_t* idx,
                               void* workspace, size_t workspace_bytes, fabhip_stream_t stream) {
    if (!log_w || !idx || !workspace || n < 1 || n_samples < 1) return FABHIP_EINVAL;
    if (order != FABHIP_ORDER_SORTED && order != FABHIP_ORDER_SHUFFLED) return FABHIP_EINVAL;
    if (n_samples > FABHIP_STRATIFIED_MAX_SAMPLES) return FABHIP_EINVAL;
    if (((size_t)workspace & 255) != 0) return FABHIP_EINVAL;
    if (workspace_bytes < fabhip_resample_stratified_workspace_bytes(n, n_samples)) return FABHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    const long ns = (long)n_samples;
    const StratWs s = carve_strat_ws(workspace, (long)n, ns);
    const EmitWs& w = s.w;
    long long* out = order == FABHIP_ORDER_SHUFFLED ? s.sorted : (long long*)idx;
    emit_front(log_w, (long)n, w, 0.0, ns, st);
    hipLaunchKernelGGL(k_emit_stratified, dim3((unsigned)w.nbk), dim3(64 * EM_NW), 0, st, log_w, (long)n, w.max_val, w.wave_sum,
                       w.block_excl, w.strata, ns, (unsigned long long)seed, out, w.strata + 4, w.giant_desc, w.giant_cap);
    return emit_finish(w, out, (long long*)idx, ns, EM_GIANT, order, (unsigned long long)seed, st);
}

}  // extern "C"
