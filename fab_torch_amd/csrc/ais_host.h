// Host-side functions one AIS unit calls in another (ais_tile16.hip, ais_tile16_metropolis.hip, ais_tile48.hip, ais_moves.hip,
// ais_driver.hip).  Every launcher enqueues on `st` and returns a FABHIP_* code; none allocates or synchronises.
#pragma once
#include "launch.h"
#include "target_device.h"
#include "ais_device.h"
#include "defensive_device.h"

namespace fab {

static inline int nblk_of(long B) { return (int)((B + ROWS - 1) / ROWS); }

// ais_tile16.hip ----------------------------------------------------------------------------------------------------------------
// chain initialisation on 16-chain tiles; `mx.on`: k_ais_init_mix with the selector `sel`
int ais_init_t16(const FlowDims& f, const float* packed, const TargetDev& tg, const float* eps0, const PointDev& pt, float* log_w,
                 float* base_log_w, fabhip_anneal an, int with_grad, long B, const MixDev& mx, const float* sel, hipStream_t st);
// one HMC outer step on 16-chain tiles (k_hmc_step, _fast or, with `mx.on`, _mix)
int hmc_step_t16(const FlowDims& f, const float* packed, const TargetDev& tg, const HmcK& a, const MixDev& mx, hipStream_t st);
// k_hmc_adapt: the step-size rule from the block partials (row_acc / row_dist: per-chain values of the 4- / 8-chain tiles)
int hmc_adapt(float* part_acc, float* part_dist, int nblk, const int* n_valid, long B, float* eps_ptr, float* ceps_ptr,
              float target_p_accept, int tune, float* p_accept_out, float* dist_out, const float* row_acc, const float* row_dist,
              float* slab, hipStream_t st);

// ais_tile16_metropolis.hip -----------------------------------------------------------------------------------------------------
// all updates of a Metropolis transition (k_metropolis or, with `mx.on`, k_metropolis_mix)
int metropolis_t16(const FlowDims& f, const float* packed, const TargetDev& tg, const MetK& a, const MixDev& mx, hipStream_t st);
// k_metropolis_adapt: the noise-scaling rule of one transition
int metropolis_adapt(const float* part_acc, int nblk, int n_updates, const int* n_valid, long B, float* scalings,
                     float target_p_accept, int tune, hipStream_t st);
// k_metropolis_count: the chains in use behind a transition's deferred block sums
int metropolis_count(const int* n_valid, long B, float* out, hipStream_t st);

// ais_tile48.hip: 4-chain tiles -------------------------------------------------------------------------------------------------
int hmc_step_r4(const FlowDims& f, const float* packed, const TargetDev& tg, const HmcK& a, hipStream_t st);
// eps0 != nullptr: the flow sample runs in the kernel as well (stream image only), else lq0 holds its log q
int ais_init_r4(const FlowDims& f, const float* packed, const TargetDev& tg, const float* lq0, const float* eps0,
                const PointDev& pt, float* log_w, float* base_log_w, fabhip_anneal an, long B, hipStream_t st);

// ais_tile48.hip: 8-chain tiles -------------------------------------------------------------------------------------------------
// whether a transition over B chains runs on 8-chain tiles (shape, LDS fit, FABHIP_OPT_TILE_SHAPE, batch size)
bool use_r8_tiles(const FlowDims& f, long B);
int hmc_step_r8(const FlowDims& f, const float* packed, const TargetDev& tg, const HmcK& a, hipStream_t st);
int ais_init_r8(const FlowDims& f, const float* packed, const TargetDev& tg, const float* lq0, const PointDev& pt, float* log_w,
                float* base_log_w, fabhip_anneal an, long B, hipStream_t st);

// ais_moves.hip -----------------------------------------------------------------------------------------------------------------
// stable compaction of the rows with finite log_p and log_q: k_valid_scan, k_compact_scatter, k_compact_copyback
int compact_rows(const fabhip_point& point, float* log_w, long B, int dim, const int* n_in, int* n_out, float* tmp, int* dest,
                 float* extra, hipStream_t st);
// SMC mode: the point gathered by the ancestors `anc` through `tmp` and back (k_smc_gather, k_smc_copyback; both read `flag`)
int smc_gather_copyback(const fabhip_point& point, float* log_w, float* tmp, const int* anc, const int* flag,
                        const float* lw_common, const int* n_ptr, long B, int dim, hipStream_t st);
// flow-proposal move: accept / commit of the proposal's Point into `cur` (k_flow_move_accept; `word` is zero before and after)
int flow_move_accept(const fabhip_point& cur, const PointDev& prop, const float* h, const int* n_ptr, long B, int dim,
                     fabhip_anneal c, unsigned long long* word, float* p_accept, int* n_accept, hipStream_t st);
// o = a - b over n floats (k_sub); the launch is not checked here
void launch_sub(const float* a, const float* b, float* o, long n, hipStream_t st);
// the spline family's initial log-weights (k_spline_init_logw); the launch is not checked here
void launch_spline_init_logw(const float* lq, const float* lp, const float* lq0, fabhip_anneal an, float* log_w,
                             float* base_log_w, long n, hipStream_t st);

// ais_driver.hip ----------------------------------------------------------------------------------------------------------------
// FABHIP_EINVAL where the point lacks x, log_q or log_p, or (need_grad) one of the two gradients
int check_point(const fabhip_point& p, bool need_grad);

}  // namespace fab
