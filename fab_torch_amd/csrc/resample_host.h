// Host-side pieces the reduction / resampler units share (reduce_kernels.hip, resample_scan.hip, resample_emit.hip,
// weight_decisions.hip): the grid helper (al256 and Bump: launch.h), and what the scan unit launches on behalf of the emit unit.
#pragma once
#include "launch.h"

namespace fab {

static inline int grid_for(long n, int threads, int cap) {
    long b = (n + threads - 1) / threads;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// resample_scan.hip -------------------------------------------------------------------------------------------------------------
// max_val[0] = the largest finite log-weight (0 when there is none), through max_part [1024]: k_max_partial, k_max_final
void launch_max(const float* log_w, long n, float* max_part, float* max_val, hipStream_t st);
// where the fabhip_resample_workspace_bytes(n) layout keeps the maximum and its (8 n)-byte CDF region
void scan_ws_regions(void* workspace, long n, float** max_part, float** max_val, unsigned long long** cdf);
// systematic resampling by scan + CDF in HBM + search, in a workspace of fabhip_resample_workspace_bytes(n)
int systematic_by_search(const float* log_w, long n, double u0, long ns, long long* idx, void* workspace, hipStream_t st);

}  // namespace fab
