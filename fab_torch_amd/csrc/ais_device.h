// Device-side pieces the AIS units share (ais_tile16.hip, ais_tile16_metropolis.hip, ais_tile48.hip, ais_moves.hip, ais_driver.hip): the
// point as the kernels see it, the argument blocks of the transition kernels and the step-size rule with its in-kernel form.
// Include it behind the flow headers a unit needs: from here on a*b+c stays un-fused, like the eager CPU reference.
#pragma once
#include "flow_device.h"

#pragma clang fp contract(off)

namespace fab {

struct PointDev {
    float *x, *lq, *lp, *gq, *gp;
};
static inline PointDev make_point_dev(const fabhip_point& p) { return PointDev{p.x, p.log_q, p.log_p, p.grad_log_q, p.grad_log_p}; }

__device__ __forceinline__ float clamp_nan0(float g, float mg) {
    // torch.nan_to_num(torch.clamp(g, -mg, mg), nan=0): NaN -> 0, +-inf -> +-mg   (hmc.py:194-199)
    return (g != g) ? 0.f : fminf(fmaxf(g, -mg), mg);
}

// ------------------------------------------------------------------------------------------------
// One HMC outer step (hmc.py:129-160): the arguments of k_hmc_step*, k_hmc_step_r4 and k_hmc_step_r8.
// ------------------------------------------------------------------------------------------------
struct HmcK {
    PointDev cur, start, prop_out;   // prop_out.x == nullptr: do not store the proposal
    long B;
    const int* n_valid;
    fabhip_anneal c, nx;
    float* log_w;                    // nullptr: no log-weight update in this launch
    const float* noise_p;            // [B][D] for this outer step
    const float* noise_e;            // [B]
    const float* eps_ptr;            // epsilons[i-1][n]
    const float* ceps_ptr;           // common_epsilon
    const float* mass;
    int L;
    float max_grad;
    float* part_acc;                 // [nblk] sum of min(1, acceptance prob)
    float* part_dist;                // [nblk] sum of the store_info distance
    float* row_acc;                  // 4-chain tiles: the same two quantities per chain [16 nblk]; k_hmc_adapt adds them
    float* row_dist;                 //   in the 16-chain kernel's order (16 rows, then blocks)
    // step-size rule inside the transition kernel (4- / 8-chain tiles of a fused AIS call; hmc_adapt_last): ticket == nullptr
    // leaves it to k_hmc_adapt
    int* ticket;                     // zero before the launch; the last wave to finish resets it
    float* eps_w;                    // = eps_ptr / ceps_ptr, writable
    float* ceps_w;
    float target_p_accept;
    int tune;
    float* p_accept_out;
    float* dist_out;
    int nblk;
};

// Metropolis transition: all n_updates for 16 chains per workgroup (metropolis.py:51-74): the arguments of k_metropolis*.
struct MetK {
    PointDev cur;
    long B;
    const int* n_valid;
    fabhip_anneal c, nx;
    float* log_w;
    const float* noise_x;            // [n_updates][B][D]
    const float* noise_u;            // [n_updates][B]
    const float* scalings;           // noise_scalings[i-1][0..n_updates)
    int n_updates;
    float* part_acc;                 // [n_updates][nblk]
    int nblk;
};

// step-size adaptation from the block partials (hmc.py:122-123,162-170), fixed summation order
// (4-chain tiles hand over per-chain values: the 64 threads first add each block's 16 rows in row order, which is
// what a 16-chain workgroup writes, so both tile shapes give the step-size rule bit-identical sums)
__device__ __forceinline__ void hmc_adapt_rule(float s, float d, long nv, float* eps_ptr, float* ceps_ptr,
                                               float target_p_accept, int tune, float* p_accept_out, float* dist_out) {
    const float log_mean = logf(s) - logf((float)nv);
    if (p_accept_out) *p_accept_out = expf(log_mean);
    if (dist_out) *dist_out = d / (float)nv;
    if (tune) {
        if (log_mean > logf(target_p_accept)) {
            *eps_ptr = *eps_ptr * 1.05f;
            *ceps_ptr = *ceps_ptr * 1.02f;
        } else {
            *eps_ptr = *eps_ptr / 1.05f;
            *ceps_ptr = *ceps_ptr / 1.02f;
        }
    }
}

// k_hmc_adapt's work (per-chain values -> blocks of 16 rows in row order -> blocks in order -> the rule: the same additions, bit
// for bit) done by the LAST wave of the launch to finish, instead of a launch of its own after every transition kernel (6 us + the
// launch gap, eight times per AIS call).  Every wave that stores row_acc / row_dist calls this once, after its stores
// (`n_waves` = such waves per workgroup).  The L2s of the 8 XCDs are not coherent with each other, and a device-scope release
// fence (buffer_wbl2) costs as much as the launch it would save (measured: +6 us per kernel): the per-chain values are written
// and read with DEVICE-SCOPE relaxed atomics instead (sc1: written through / read past the XCD's L2), the wave waits for its
// stores (vmcnt) before it draws its ticket, and the wave that draws the last one sums and applies the rule.  Nobody reads the
// step sizes any more by then (every workgroup loads them at its top); the next launch sees the new ones.
// `scratch`: 2 nblk floats of LDS that no wave of this workgroup still reads.
__device__ __forceinline__ void hmc_store_row_stats(const HmcK& a, long g, float contrib, float dist) {
    if (a.ticket) {
        __hip_atomic_store(a.row_acc + g, contrib, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.row_dist + g, dist, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        a.row_acc[g] = contrib; a.row_dist[g] = dist;
    }
}
__device__ __forceinline__ void hmc_adapt_last(const HmcK& a, float* scratch, int lane, int n_waves) {
    if (!a.ticket) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    int tk = 0;
    if (lane == 0) tk = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tk = __builtin_amdgcn_readfirstlane(tk);
    if (tk != (int)gridDim.x * n_waves - 1) return;
    const int nblk = a.nblk;
    for (int b = lane; b < nblk; b += 64) {
        float s = 0.f, d = 0.f;
        for (int r = 0; r < ROWS; ++r) {
            s += __hip_atomic_load(a.row_acc + (long)b * ROWS + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            d += __hip_atomic_load(a.row_dist + (long)b * ROWS + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        scratch[b] = s; scratch[nblk + b] = d;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // one wave: its LDS writes are done before lane 0 reads them
    if (lane == 0) {
        const long nv = a.n_valid ? (long)*a.n_valid : a.B;
        if (nv > 0) {
            float s = 0.f, d = 0.f;
            for (int i = 0; i < nblk; ++i) { s += scratch[i]; d += scratch[nblk + i]; }
            hmc_adapt_rule(s, d, nv, a.eps_w, a.ceps_w, a.target_p_accept, a.tune, a.p_accept_out, a.dist_out);
        }
        __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace fab
