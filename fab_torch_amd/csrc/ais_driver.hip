// The AIS call on the host: workspace layouts, the HMC / Metropolis transition drivers, the phases of the fused AIS call
// (RealNVP family) and the fused spline AIS call.  No kernel lives here: every launch goes through ais_host.h.
#include "flow_device.h"
#include "target_device.h"
#include "launch.h"

#pragma clang fp contract(off)

#include "ais_device.h"
#include "ais_host.h"

namespace fab {

// ---- workspace layouts (launch.h: Bump; sizes = carve(nullptr, ..).bytes) -------------------------------------------------------
struct HmcWs {
    float *part_acc, *part_dist;       // [nblk] block partials
    float *row_acc, *row_dist;         // [16 nblk] per-chain values (4- / 8-chain tiles)
    PointDev prop;                     // n_outer > 1: the proposal the next outer step starts from (else null)
    size_t bytes;
};
static HmcWs carve_hmc_ws(void* workspace, long B, int D, int n_outer) {
    HmcWs w;
    const size_t nblk = (size_t)nblk_of(B);
    Bump b{(char*)workspace, 256};
    w.part_acc = b.take<float>(nblk);
    w.part_dist = b.take<float>(nblk);
    w.row_acc = b.take<float>(nblk * ROWS);
    w.row_dist = b.take<float>(nblk * ROWS);
    w.prop = PointDev{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (n_outer > 1) {
        float* pb = b.take<float>((size_t)B * (3 * D + 2));
        w.prop.x = pb; w.prop.gq = pb + B * D; w.prop.gp = pb + 2 * B * D;
        w.prop.lq = pb + 3 * B * D; w.prop.lp = w.prop.lq + B;
    }
    w.bytes = (size_t)(b.p - (char*)workspace) + 256;
    return w;
}

struct AisWs {
    void* trans_ws;                    // the transition's own workspace (HMC or Metropolis, whichever is larger)
    size_t trans_bytes;
    float* tmp;                        // [B][3D+4] compaction staging
    int* dest;                         // [B] dest ranks
    float* lwb;                        // [B] log_p - log_q
    void* ess_ws;
    size_t ess_bytes;
    int* ticket;                       // the word of the in-kernel step-size rule
    // SMC scratch, behind the plain call's layout (which it leaves as it is); null unless the mode is on
    unsigned long long* smc_cdf;       // [B]
    int *smc_anc, *smc_flag;           // [B], [1]
    float* smc_lw;                     // [1]
    // flow-proposal moves, behind all of it; null unless the mode is on
    unsigned long long* mv_word;       // the accept kernel's count word
    float* mv_prop;                    // [B][3D+2] the proposal's Point
    size_t bytes;
};
// the proposal's Point inside a [B][3D+2] buffer: x | grad log q | grad log p | log q | log p (gradients null when !with_grad)
static PointDev prop_point(float* pb, long B, int D, bool with_grad) {
    return PointDev{pb, pb + 3 * B * D, pb + 3 * B * D + B, with_grad ? pb + B * D : nullptr, with_grad ? pb + 2 * B * D : nullptr};
}
// The optional modes of one fused call (include/fabhip.h: fabhip_ais_ext) and which of them are on.  The size function and the
// call both resolve their `ext` here, so that size and carve cannot disagree.
struct AisModes {
    const fabhip_smc_args* smc;
    const fabhip_defensive_args* mix;
    const fabhip_flow_moves_args* moves;
    bool smc_on, mv_on;
    MixDev mx;                         // mx.on: the defensive mixture
};
static AisModes resolve_ext(const fabhip_ais_ext* ext) {
    AisModes m{};
    if (ext) { m.smc = ext->smc; m.mix = ext->mix; m.moves = ext->moves; }
    m.smc_on = m.smc && m.smc->enabled != 0;
    m.mv_on = m.moves && m.moves->n_moves > 0;
    m.mx = make_mix_dev(m.mix);
    return m;
}
static AisWs carve_ais_ws(void* workspace, long B, int D, int n_inner, const AisModes& m) {
    AisWs w{};
    size_t tws = fabhip_hmc_workspace_bytes(B, D, n_inner);
    const size_t mws = fabhip_metropolis_workspace_bytes(B, D, n_inner);
    if (mws > tws) tws = mws;
    Bump b{(char*)workspace, 256};
    w.trans_bytes = al256(tws);
    w.trans_ws = b.take<char>(w.trans_bytes);
    w.tmp = b.take<float>((size_t)B * (3 * D + 4));
    w.dest = b.take<int>((size_t)B);
    w.lwb = b.take<float>((size_t)B);
    w.ess_bytes = fabhip_ess_workspace_bytes(B);
    w.ess_ws = b.take<char>(w.ess_bytes);
    w.ticket = b.take<int>(1);
    b.take<char>(256);                 // slack
    if (m.smc_on) {
        w.smc_cdf = b.take<unsigned long long>((size_t)B);
        w.smc_anc = b.take<int>((size_t)B);
        char* p = b.take<char>(256);
        w.smc_flag = (int*)p;
        w.smc_lw = (float*)(p + 64);
    }
    if (m.mv_on) {
        w.mv_word = b.take<unsigned long long>(1);
        w.mv_prop = b.take<float>((size_t)B * (3 * D + 2));
    }
    w.bytes = (size_t)(b.p - (char*)workspace);
    return w;
}

struct FlowMoveWs {
    unsigned long long* word;
    float* prop;                       // [B][3D+2]
    size_t bytes;
};
static FlowMoveWs carve_flow_move_ws(void* workspace, long B, int D) {
    FlowMoveWs w;
    Bump b{(char*)workspace, 256};
    w.word = b.take<unsigned long long>(1);
    w.prop = b.take<float>((size_t)B * (3 * D + 2));
    w.bytes = (size_t)(b.p - (char*)workspace);
    return w;
}

// One flow-proposal move (include/fabhip.h: fabhip_flow_move): sample, create_point, accept / commit.  `word` is zero.
static int flow_move_impl(const fabhip_flow& flow, const fabhip_target& target, const fabhip_point& point, long B, const int* n_valid,
                          fabhip_anneal c, const float* noise_g, const float* noise_h, float* p_accept, int* n_accept,
                          unsigned long long* word, float* prop_buf, hipStream_t st) {
    const int D = flow.dim;
    const bool with_grad = point.grad_log_q != nullptr;
    const PointDev pd = prop_point(prop_buf, B, D, with_grad);
    const fabhip_point prop{pd.x, pd.lq, pd.lp, pd.gq, pd.gp};
    FAB_TRY(fabhip_flow_sample(&flow, noise_g, prop.x, prop.log_q, B, (fabhip_stream_t)st));
    FAB_TRY(fabhip_create_point(&flow, &target, &prop, with_grad ? 1 : 0, B, (fabhip_stream_t)st));
    return flow_move_accept(point, pd, noise_h, n_valid, B, D, c, word, p_accept, n_accept, st);
}

struct SplineHmcWs {
    void *gen_ws, *spline_ws;          // generic-HMC state, the spline kernels' own scratch
    size_t gen_bytes, spline_bytes;
    float* prop;                       // [B][3D+2] the proposal
    float *row_acc, *row_dist;         // [16 nblk] the fold's per-chain values
    int* ticket;                       // the fold's ticket word, behind them
    size_t bytes;
};
static SplineHmcWs carve_spline_hmc_ws(void* workspace, int D, int n_layers, int hidden, long B) {
    SplineHmcWs w;
    Bump b{(char*)workspace, 256};
    w.gen_bytes = fabhip_generic_workspace_bytes(B, D);
    w.gen_ws = b.take<char>(w.gen_bytes);
    w.spline_bytes = fabhip_spline_workspace_bytes(D, n_layers, hidden, B, 1);
    w.spline_ws = b.take<char>(w.spline_bytes);
    w.prop = b.take<float>((size_t)B * (3 * D + 2));
    const size_t nblk = (size_t)((B + 15) / 16);
    w.row_acc = b.take<float>(spline_fold_scratch_floats(B));
    w.row_dist = w.row_acc + 16 * nblk;
    w.ticket = (int*)(w.row_acc + 32 * nblk);
    w.bytes = (size_t)(b.p - (char*)workspace) + 256;
    return w;
}

struct SplineAisWs {
    void* trans_ws;                    // the transition's workspace (carve_spline_hmc_ws)
    size_t trans_bytes;
    float* tmp;                        // [B][3D+4] compaction staging
    int* dest;                         // [B] dest ranks
    float *lwb, *lq0;                  // [B] log_p - log_q, [B] log q of the sampling pass
    void* ess_ws;
    size_t ess_bytes;
    size_t bytes;
};
static SplineAisWs carve_spline_ais_ws(void* workspace, int D, int n_layers, int hidden, long B) {
    SplineAisWs w;
    Bump b{(char*)workspace, 256};
    w.trans_bytes = al256(fabhip_spline_hmc_workspace_bytes(D, n_layers, hidden, B));
    w.trans_ws = b.take<char>(w.trans_bytes);
    w.tmp = b.take<float>((size_t)B * (3 * D + 4));
    w.dest = b.take<int>((size_t)B);
    w.lwb = b.take<float>((size_t)B);
    w.lq0 = b.take<float>((size_t)B);
    w.ess_bytes = fabhip_ess_workspace_bytes(B);
    w.ess_ws = b.take<char>(w.ess_bytes);
    w.bytes = (size_t)(b.p - (char*)workspace) + 256;
    return w;
}

// `mx.on`: the defensive mixture - 16-chain tiles at every batch size, the step-size rule in k_hmc_adapt
static int hmc_transition_impl(const fabhip_hmc_args* a, hipStream_t st, int* ticket = nullptr, const MixDev& mx = MixDev{}) {
    const FlowDims f = flow_dims_of(a->flow);
    const TargetDev tg = make_target_dev(a->target);
    const int D = f.D;
    const int nblk = nblk_of(a->B);
    const HmcWs w = carve_hmc_ws(a->workspace, a->B, D, a->n_outer);
    if (a->workspace_bytes < w.bytes) return FABHIP_ENOSPC;
    if (a->partials && a->n_outer != 1) return FABHIP_ENOTSUP;      // (the next outer loop needs the adapted common_epsilon)
    const bool r8 = !mx.on && use_r8_tiles(f, a->B);
    const bool r4 = !mx.on && !r8 && use_r4_tiles(f, a->B);
    const PointDev cur = make_point_dev(a->point);
    for (int n = 0; n < a->n_outer; ++n) {
        HmcK k;
        k.cur = cur;
        k.start = (n == 0) ? cur : w.prop;
        k.prop_out = (n + 1 < a->n_outer) ? w.prop : PointDev{nullptr, nullptr, nullptr, nullptr, nullptr};
        k.B = a->B; k.n_valid = a->n_valid; k.c = a->cur; k.nx = a->next;
        k.log_w = (n + 1 == a->n_outer) ? a->log_w : nullptr;
        k.noise_p = a->noise_p + (size_t)n * a->B * D;
        k.noise_e = a->noise_e + (size_t)n * a->B;
        k.eps_ptr = a->epsilons + n; k.ceps_ptr = a->common_epsilon; k.mass = a->mass;
        k.L = a->L; k.max_grad = a->max_grad; k.part_acc = w.part_acc; k.part_dist = w.part_dist;
        k.row_acc = w.row_acc; k.row_dist = w.row_dist;
        // the step-size rule in the transition kernel's last workgroup (4- / 8-chain tiles; `ticket` is zero: fabhip_ais_phase)
        const bool fold = ticket && (r4 || r8) && !a->partials;
        k.ticket = fold ? ticket : nullptr;
        k.eps_w = a->epsilons + n; k.ceps_w = a->common_epsilon; k.target_p_accept = a->target_p_accept; k.tune = a->tune;
        k.p_accept_out = a->p_accept ? a->p_accept + n : nullptr; k.dist_out = a->avg_distance; k.nblk = nblk;
        if (mx.on) FAB_TRY(hmc_step_t16(f, a->flow.packed, tg, k, mx, st));
        else if (r8) FAB_TRY(hmc_step_r8(f, a->flow.packed, tg, k, st));
        else if (r4) FAB_TRY(hmc_step_r4(f, a->flow.packed, tg, k, st));
        else FAB_TRY(hmc_step_t16(f, a->flow.packed, tg, k, MixDev{}, st));
        if (fold) { FAB_TRY(check_launch()); continue; }
        FAB_TRY(hmc_adapt(w.part_acc, w.part_dist, nblk, a->n_valid, (long)a->B, a->epsilons + n, a->common_epsilon,
                          a->target_p_accept, a->tune, a->p_accept ? a->p_accept + n : nullptr, a->avg_distance,
                          (r4 || r8) ? w.row_acc : (const float*)nullptr, (r4 || r8) ? w.row_dist : (const float*)nullptr,
                          a->partials, st));
    }
    return FABHIP_OK;
}

static int metropolis_transition_impl(const fabhip_metropolis_args* a, hipStream_t st, float* partials = nullptr,
                                      const MixDev& mx = MixDev{}) {
    const FlowDims f = flow_dims_of(a->flow);
    const TargetDev tg = make_target_dev(a->target);
    const int nblk = nblk_of(a->B);
    if (a->workspace_bytes < fabhip_metropolis_workspace_bytes(a->B, f.D, a->n_updates)) return FABHIP_ENOSPC;
    MetK k;
    k.cur = make_point_dev(a->point); k.B = a->B; k.n_valid = a->n_valid; k.c = a->cur; k.nx = a->next;
    k.log_w = a->log_w; k.noise_x = a->noise_x; k.noise_u = a->noise_u; k.scalings = a->noise_scalings;
    k.n_updates = a->n_updates; k.part_acc = partials ? partials : (float*)a->workspace; k.nblk = nblk;
    FAB_TRY(metropolis_t16(f, a->flow.packed, tg, k, mx, st));
    if (partials)                    // deferred rule (sharded chains): [n_updates][nblk] block sums | chains in use
        return metropolis_count(a->n_valid, (long)a->B, partials + (size_t)a->n_updates * nblk, st);
    return metropolis_adapt(k.part_acc, nblk, a->n_updates, a->n_valid, (long)a->B, a->noise_scalings, a->target_p_accept,
                            a->tune, st);
}

int check_point(const fabhip_point& p, bool need_grad) {
    if (!p.x || !p.log_q || !p.log_p) return FABHIP_EINVAL;
    if (need_grad && (!p.grad_log_q || !p.grad_log_p)) return FABHIP_EINVAL;
    return FABHIP_OK;
}

// the tail of a chain phase: compaction (+ log_p - log_q) + ESS / log Z - one launch for small batches, else the separate kernels
static int phase_tail(const fabhip_point& point, float* log_w, long B, int dim, const int* n_in, int* n_out, float* tmp, int* dest,
                      float* extra, float* diff, double n_norm, float* stats_out, void* ess_ws, size_t ess_bytes, float* base_x,
                      int* zero_word, float* zero_f, hipStream_t st) {
    int rc = FABHIP_ENOTSUP;
    if (option(FABHIP_OPT_FUSED_TAIL) != 0) {
        TailArgs t;
        t.x = point.x; t.lq = point.log_q; t.lp = point.log_p; t.gq = point.grad_log_q; t.gp = point.grad_log_p;
        t.log_w = log_w; t.extra = extra; t.n_in = n_in; t.n_out = n_out; t.B = B; t.D = dim; t.diff = diff; t.n_norm = n_norm;
        t.stats_out = stats_out; t.zero_word = zero_word; t.zero_f = zero_f; t.n_zero_f = zero_f ? 10 : 0;
        rc = tail_small(t, dest, st);
        if (rc != FABHIP_OK && rc != FABHIP_ENOTSUP) return rc;
    }
    if (rc == FABHIP_ENOTSUP) {
        if (zero_word && hipMemsetAsync(zero_word, 0, 4, st) != hipSuccess) return FABHIP_ELAUNCH;
        if (zero_f && hipMemsetAsync(zero_f, 0, 10 * 4, st) != hipSuccess) return FABHIP_ELAUNCH;
        FAB_TRY(compact_rows(point, log_w, B, dim, n_in, n_out, tmp, dest, extra, st));
    }
    if (base_x &&         // the compacted starting points (rows beyond the count are don't-care)
        hipMemcpyAsync(base_x, point.x, (size_t)B * dim * 4, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return FABHIP_ELAUNCH;
    if (rc == FABHIP_ENOTSUP) {
        if (diff) launch_sub(point.log_p, point.log_q, diff, B, st);
        FAB_TRY(fabhip_ess_logz(diff ? diff : log_w, B, n_out, n_norm, stats_out, ess_ws, ess_bytes, (fabhip_stream_t)st));
    }
    return check_launch();
}

// ---- the fused AIS call (RealNVP family), step by step; fabhip_ais_phase_ext strings the steps together ---------------------------
// The argument checks of a call that runs `phases` and the transitions j_begin .. j_end, in the precedence of their return codes
// (the workspace size comes behind them: the caller carves with `*modes`).
static int check_ais_call(const fabhip_ais_args* a, const fabhip_ais_ext* ext, int32_t phases, int32_t j_begin, int32_t j_end,
                          const float* partials, AisModes* modes) {
    if (!a || !a->flow.packed || !a->betas || !a->step_state || !a->log_w ||
        !a->n_valid || !a->stats || !a->workspace || a->B < 1 || a->M < 1 || a->n_inner < 1)
        return FABHIP_EINVAL;
    if (j_begin <= j_end && (!a->noise_a || !a->noise_b)) return FABHIP_EINVAL;       // (read by the transitions only)
    const bool do_init = (phases & FABHIP_AIS_INIT) != 0;
    if (do_init && !a->eps0) return FABHIP_EINVAL;
    if (j_begin <= j_end && (j_begin < 1 || j_end > a->M)) return FABHIP_EINVAL;
    if (partials && a->transition == FABHIP_TRANSITION_HMC && j_begin != j_end) return FABHIP_ENOTSUP;
    const bool hmc = a->transition == FABHIP_TRANSITION_HMC;
    if (!hmc && a->transition != FABHIP_TRANSITION_METROPOLIS) return FABHIP_EINVAL;
    if (hmc && (!a->common_epsilon || !a->mass)) return FABHIP_EINVAL;
    FAB_TRY(check_flow_shape(a->flow.dim, a->flow.n_layers, a->flow.width));
    FAB_TRY(check_target(&a->target, a->flow.dim));
    FAB_TRY(check_point(a->point, hmc));
    const AisModes m = resolve_ext(ext);
    FAB_TRY(check_mix(m.mix));
    if (m.mx.on && (partials || resolve_fast(a->flow.precision))) return FABHIP_ENOTSUP;  // (sharded chains, bf16 fast mode)
    if (m.mx.on && do_init && !m.mix->sel) return FABHIP_EINVAL;                          // (like eps0: read by INIT only)
    if (m.smc_on && partials) return FABHIP_ENOTSUP;
    if (m.smc_on && m.smc->method != FABHIP_SMC_SYSTEMATIC && m.smc->method != FABHIP_SMC_STRATIFIED) return FABHIP_EINVAL;
    if (m.smc_on && j_begin <= j_end && !m.smc->u) return FABHIP_EINVAL;              // (like the noise: read by the transitions only)
    if (m.moves && m.moves->n_moves < 0) return FABHIP_EINVAL;
    if (m.mv_on && (partials || m.mx.on)) return FABHIP_ENOTSUP;                      // (sharded chains, defensive mixture)
    if (m.mv_on && j_begin <= j_end && (!m.moves->noise_g || !m.moves->noise_h)) return FABHIP_EINVAL;
    if (m.mv_on && a->B > 0x3fffffffL) return FABHIP_EINVAL;
    *modes = m;
    return FABHIP_OK;
}

// what the steps of one call share
struct AisCall {
    const fabhip_ais_args* a;
    AisModes m;
    AisWs w;
    FlowDims f;
    TargetDev tg;
    bool hmc;
    int* ticket;                       // the word of the in-kernel step-size rule (hmc_adapt_last), or null: k_hmc_adapt launches
    float* partials;
    hipStream_t st;
};

// 1. chain initialisation, 2. remove nan/inf ("chain init"), 3. ESS over the base samples (ais.py:68-71) -> stats[0..2]
static int ais_chain_init(const AisCall& c) {
    const fabhip_ais_args* a = c.a;
    const AisWs& w = c.w;
    const FlowDims& f = c.f;
    const long B = a->B;
    const int hmc = c.hmc ? 1 : 0;
    fabhip_anneal a1;
    fabhip_anneal_coefs(a->betas[1], a->alpha, a->p_target, &a1);
    const PointDev pt = make_point_dev(a->point);
    if (c.m.mx.on) {
        FAB_TRY(ais_init_t16(f, a->flow.packed, c.tg, a->eps0, pt, a->log_w, a->base_log_w, a1, hmc, B, c.m.mx, c.m.mix->sel, c.st));
    } else if (hmc && use_r8_tiles(f, B)) {
        FAB_TRY(fabhip_flow_sample(&a->flow, a->eps0, a->point.x, w.lwb, B, (fabhip_stream_t)c.st));
        FAB_TRY(ais_init_r8(f, a->flow.packed, c.tg, w.lwb, pt, a->log_w, a->base_log_w, a1, B, c.st));
    } else if (hmc && use_r4_tiles(f, B) && option(FABHIP_OPT_R4_STREAM) != 0) {
        // 4-chain tiles: x, log q0 = flow.sample(eps0), then log q + d/dx (the reference re-evaluates: base.py:65-68), target,
        // log w - one kernel where the stream image exists (f.o_r4s), else the flow-sample kernel first
        if (f.o_r4s >= 0 && f.NTW / 4 >= 2) {
            FAB_TRY(ais_init_r4(f, a->flow.packed, c.tg, nullptr, a->eps0, pt, a->log_w, a->base_log_w, a1, B, c.st));
        } else {
            FAB_TRY(fabhip_flow_sample(&a->flow, a->eps0, a->point.x, w.lwb, B, (fabhip_stream_t)c.st));
            FAB_TRY(ais_init_r4(f, a->flow.packed, c.tg, w.lwb, nullptr, pt, a->log_w, a->base_log_w, a1, B, c.st));
        }
    } else {
        FAB_TRY(ais_init_t16(f, a->flow.packed, c.tg, a->eps0, pt, a->log_w, a->base_log_w, a1, hmc, B, MixDev{}, nullptr, c.st));
    }
    return phase_tail(a->point, a->log_w, B, f.D, nullptr, a->n_valid, w.tmp, w.dest, a->base_log_w, w.lwb, 1.0, a->stats + 0,
                      w.ess_ws, w.ess_bytes, a->base_x, c.ticket, a->stats + 6, c.st);
}

// resampling step of transition j (log_w targets the distribution this transition leaves invariant): decision,
// gather into the staging buffer, copy back - three launches whatever the decision.  No transition kernel keeps
// per-chain state in the workspace from one transition to the next (part_* / row_* / the proposal buffer are
// written and consumed inside one transition), so the point and log_w are all there is to move.
static int ais_resample_step(const AisCall& c, int j) {
    const fabhip_ais_args* a = c.a;
    const fabhip_smc_args* smc = c.m.smc;
    const AisWs& w = c.w;
    const long B = a->B;
    SmcK k;
    k.log_w = a->log_w; k.n_ptr = a->n_valid; k.B = B; k.tau = smc->tau; k.u = smc->u + (j - 1);
    k.cdf = w.smc_cdf; k.anc = w.smc_anc; k.flag = w.smc_flag; k.lw_common = w.smc_lw;
    k.resampled_out = smc->resampled ? smc->resampled + (j - 1) : nullptr;
    k.ess_out = smc->ess ? smc->ess + (j - 1) : nullptr;
    k.anc_out = smc->ancestors ? smc->ancestors + (size_t)(j - 1) * B : nullptr;
    k.lw_pre_out = smc->log_w_pre ? smc->log_w_pre + (size_t)(j - 1) * B : nullptr;
    k.method = smc->method;
    FAB_TRY(smc_decide(k, c.st));
    return smc_gather_copyback(a->point, a->log_w, w.tmp, w.smc_anc, w.smc_flag, w.smc_lw, a->n_valid, B, c.f.D, c.st);
}

// global moves of step j at beta_j (coefficients `cj`), behind the resampling step and in front of the local transition: three
// launches each; they neither read nor write log_w, the step sizes or the ticket word
static int ais_moves_step(const AisCall& c, int j, fabhip_anneal cj) {
    const fabhip_ais_args* a = c.a;
    const fabhip_flow_moves_args* moves = c.m.moves;
    const long B = a->B;
    const int D = c.f.D, k = moves->n_moves;
    for (int m = 0; m < k; ++m) {
        const size_t slab = (size_t)(j - 1) * k + m;
        FAB_TRY(flow_move_impl(a->flow, a->target, a->point, B, a->n_valid, cj, moves->noise_g + slab * B * D,
                               moves->noise_h + slab * B, moves->p_accept_out ? moves->p_accept_out + slab : nullptr,
                               nullptr, c.w.mv_word, c.w.mv_prop, c.st));
    }
    return FABHIP_OK;
}

// transition j, HMC or Metropolis, from beta_j (`cj`) towards beta_{j+1} (`cn`)
static int ais_transition(const AisCall& c, int j, fabhip_anneal cj, fabhip_anneal cn) {
    const fabhip_ais_args* a = c.a;
    const AisWs& w = c.w;
    const long B = a->B;
    const int D = c.f.D;
    float* lw = (a->betas[j + 1] != a->betas[j]) ? a->log_w : nullptr;      // ais.py:93
    const size_t nslab = (size_t)(j - 1) * a->n_inner;
    if (c.hmc) {
        fabhip_hmc_args h;
        h.flow = a->flow; h.target = a->target; h.point = a->point; h.B = B; h.n_valid = a->n_valid;
        h.cur = cj; h.next = cn; h.log_w = lw;
        h.noise_p = a->noise_a + nslab * B * D; h.noise_e = a->noise_b + nslab * B;
        h.epsilons = a->step_state + nslab; h.common_epsilon = a->common_epsilon; h.mass = a->mass;
        h.n_outer = a->n_inner; h.L = a->L; h.max_grad = a->max_grad; h.target_p_accept = a->target_p_accept;
        h.tune = a->tune;
        h.p_accept = nullptr; h.avg_distance = nullptr;
        h.workspace = w.trans_ws; h.workspace_bytes = w.trans_bytes;
        h.partials = c.partials;
        // logging slots of the first / last distribution (hmc.py:173-183), one acceptance per outer loop
        if (j == 1) { h.p_accept = a->p_accept_first; h.avg_distance = a->avg_distance_first; }
        else if (j == a->M) { h.p_accept = a->p_accept_last; h.avg_distance = a->avg_distance_last; }
        return hmc_transition_impl(&h, c.st, c.ticket, c.m.mx);
    }
    fabhip_metropolis_args m;
    m.flow = a->flow; m.target = a->target; m.point = a->point; m.B = B; m.n_valid = a->n_valid;
    m.cur = cj; m.next = cn; m.log_w = lw;
    m.noise_x = a->noise_a + nslab * B * D; m.noise_u = a->noise_b + nslab * B;
    m.noise_scalings = a->step_state + nslab; m.n_updates = a->n_inner;
    m.target_p_accept = a->target_p_accept; m.tune = a->tune;
    m.workspace = w.trans_ws; m.workspace_bytes = w.trans_bytes;
    // deferred rule: transition j's block sums + count at slab offset (j - 1) (n_updates nblk + 1)
    return metropolis_transition_impl(&m, c.st, c.partials ? c.partials + (size_t)(j - 1) * ((size_t)a->n_inner * nblk_of(B) + 1)
                                                           : nullptr, c.m.mx);
}

// 5. remove nan/inf ("chain end"), 6. ESS / log Z over the survivors (ais.py:77-86) -> stats[3..5]
static int ais_finish(const AisCall& c) {
    const fabhip_ais_args* a = c.a;
    return phase_tail(a->point, a->log_w, a->B, c.f.D, a->n_valid, a->n_valid + 1, c.w.tmp, c.w.dest, nullptr, nullptr, (double)a->B,
                      a->stats + 3, c.w.ess_ws, c.w.ess_bytes, nullptr, nullptr, nullptr, c.st);
}

}  // namespace fab

using namespace fab;

extern "C" {

void fabhip_anneal_coefs(double beta, double alpha, int32_t p_target, fabhip_anneal* out) {
    if (!out) return;
    if (!p_target) {   // base.py:93-94, 114-116
        out->c_q = (float)((1.0 - beta) + beta * (1.0 - alpha));
        out->c_p = (float)(beta * alpha);
        out->g_q = out->c_q;
        out->g_p = (float)(2.0 * beta);
    } else {           // base.py:96-97, 117-118
        out->c_q = (float)(1.0 - beta);
        out->c_p = (float)beta;
        out->g_q = out->c_q;
        out->g_p = out->c_p;
    }
}

size_t fabhip_hmc_workspace_bytes(int64_t B, int32_t dim, int32_t n_outer) { return carve_hmc_ws(nullptr, B, dim, n_outer).bytes; }

int fabhip_hmc_transition(const fabhip_hmc_args* a, fabhip_stream_t stream) {
    if (!a || !a->flow.packed || !a->noise_p || !a->noise_e || !a->epsilons || !a->common_epsilon || !a->mass ||
        !a->workspace || a->B < 0 || a->n_outer < 1 || a->L < 0)
        return FABHIP_EINVAL;
    FAB_TRY(check_flow_shape(a->flow.dim, a->flow.n_layers, a->flow.width));
    FAB_TRY(check_target(&a->target, a->flow.dim));
    FAB_TRY(check_point(a->point, true));
    if (a->B == 0) return FABHIP_OK;
    return hmc_transition_impl(a, (hipStream_t)stream);
}

size_t fabhip_metropolis_workspace_bytes(int64_t B, int32_t dim, int32_t n_updates) {
    (void)dim;
    return al256((size_t)nblk_of(B) * (size_t)(n_updates > 0 ? n_updates : 1) * 4) + 256;
}

int fabhip_metropolis_transition(const fabhip_metropolis_args* a, fabhip_stream_t stream) {
    if (!a || !a->flow.packed || !a->noise_x || !a->noise_u || !a->noise_scalings || !a->workspace || a->B < 0 ||
        a->n_updates < 1)
        return FABHIP_EINVAL;
    FAB_TRY(check_flow_shape(a->flow.dim, a->flow.n_layers, a->flow.width));
    FAB_TRY(check_target(&a->target, a->flow.dim));
    FAB_TRY(check_point(a->point, false));
    if (a->B == 0) return FABHIP_OK;
    return metropolis_transition_impl(a, (hipStream_t)stream);
}

// ---- whole AIS call -------------------------------------------------------------------------------
size_t fabhip_ais_workspace_bytes(int64_t B, int32_t dim, int32_t n_inner) { return fabhip_ais_ext_workspace_bytes(B, dim, n_inner, nullptr); }

size_t fabhip_ais_ext_workspace_bytes(int64_t B, int32_t dim, int32_t n_inner, const fabhip_ais_ext* ext) {
    return carve_ais_ws(nullptr, B, dim, n_inner, resolve_ext(ext)).bytes;
}

// ---- spline flow as base distribution (csrc/spline_stream.hip, spline_tile16.hip) ------------------------------------------------------
size_t fabhip_spline_hmc_workspace_bytes(int32_t dim, int32_t n_layers, int32_t hidden, int64_t B) {
    return carve_spline_hmc_ws(nullptr, dim, n_layers, hidden, B).bytes;
}

// `ticket_zeroed`: the caller has already zeroed the fold's ticket word in this workspace (fabhip_spline_ais_run: once per call;
// the wave that draws the last ticket of a launch resets it)
static int spline_hmc_transition_impl(const fabhip_spline_hmc_args* a, fabhip_stream_t stream, bool ticket_zeroed) {
    if (!a || !a->flow.packed || !a->noise_p || !a->noise_e || !a->epsilons || !a->common_epsilon || !a->mass ||
        !a->workspace || a->B < 0 || a->n_outer < 1 || a->L < 1)
        return FABHIP_EINVAL;
    FAB_TRY(check_target(&a->target, a->flow.dim));
    FAB_TRY(check_point(a->point, true));
    const int D = a->flow.dim;
    const long B = a->B;
    const SplineHmcWs w = carve_spline_hmc_ws(a->workspace, D, a->flow.n_layers, a->flow.hidden, B);
    if (a->workspace_bytes < w.bytes) return FABHIP_ENOSPC;
    if (B == 0) return FABHIP_OK;
    hipStream_t st = (hipStream_t)stream;
    void* gws = w.gen_ws;
    const size_t gb = w.gen_bytes;
    void* sws = w.spline_ws;
    const size_t sb = w.spline_bytes;
    float* pb = w.prop;
    fabhip_point prop{pb, pb + 3 * B * D, pb + 3 * B * D + B, pb + B * D, pb + 2 * B * D};
    const fabhip_point cur = a->point;
    fabhip_point start = cur;
    // round 5: begin / accept / step-size rule inside the first / last leapfrog launch (L launches per outer step instead of
    // L + 3) where the one-launch leapfrog applies - the same arithmetic in the same order, bit for bit (spline_r8.h)
    const bool fold = spline_leap_fold_supported(&a->flow, B);
    const int nblk = (int)((B + 15) / 16);
    if (fold && !ticket_zeroed && hipMemsetAsync(w.ticket, 0, 4, st) != hipSuccess) return FABHIP_ELAUNCH;
    for (int n = 0; n < a->n_outer; ++n) {
        const bool last = n + 1 == a->n_outer;
        if (!fold)
            FAB_TRY(gen_hmc_begin(&start, &cur, B, D, a->cur, a->noise_p + (size_t)n * B * D, a->mass, a->max_grad, gws, a->n_valid, st));
        for (int l = 0; l < a->L; ++l) {
            {   // one launch per leapfrog where the 4x4x1 spline kernel applies (launch.h: SplineLeap)
                float *XPw, *Pw, *GUw;
                gen_hmc_state(gws, B, D, &XPw, &Pw, &GUw);
                SplineLeap lp;
                lp.fold = SplineFold{};
                if (fold) {
                    SplineFold& fd = lp.fold;
                    fd.flags = (l == 0 ? 1 : 0) | (l + 1 == a->L ? 2 : 0);
                    fd.start_x = start.x; fd.start_gq = start.grad_log_q; fd.start_gp = start.grad_log_p;
                    fd.noise_p = a->noise_p + (size_t)n * B * D;
                    fd.logp_cur = GUw + (size_t)B * D;              // the generic workspace's per-chain row (generic_kernels.hip: split_ws)
                    fd.cur_x = cur.x; fd.cur_lq = cur.log_q; fd.cur_lp = cur.log_p; fd.cur_gq = cur.grad_log_q; fd.cur_gp = cur.grad_log_p;
                    fd.noise_e = a->noise_e + (size_t)n * B; fd.nx = a->next; fd.log_w = last ? a->log_w : nullptr;
                    fd.n_valid = a->n_valid; fd.row_acc = w.row_acc; fd.row_dist = w.row_dist;
                    fd.ticket = w.ticket;
                    fd.eps_w = a->epsilons + n; fd.ceps_w = a->common_epsilon; fd.target_p_accept = a->target_p_accept; fd.tune = a->tune;
                    fd.p_accept_out = a->p_accept ? a->p_accept + n : nullptr; fd.dist_out = a->avg_distance; fd.nblk = nblk;
                }
                lp.XP = XPw; lp.x_out = prop.x; lp.P = Pw; lp.GU = GUw; lp.eps_ptr = a->epsilons + n; lp.ceps_ptr = a->common_epsilon; lp.mass = a->mass;
                lp.c = a->cur; lp.max_grad = a->max_grad; lp.tg = a->target; lp.prop_lp = prop.log_p; lp.prop_gp = prop.grad_log_p;
                const int rc = spline_log_prob_leap(&a->flow, lp, prop.log_q, prop.grad_log_q, B, sws, sb, st);
                if (rc == FABHIP_OK) continue;
                if (rc != FABHIP_ENOTSUP || fold) return rc == FABHIP_ENOTSUP ? FABHIP_EINVAL : rc;
            }
            FAB_TRY(fabhip_hmc_generic_leap_pre(B, D, a->epsilons + n, a->common_epsilon, a->mass, prop.x, gws, gb, stream));
            FAB_TRY(fabhip_spline_log_prob(&a->flow, prop.x, prop.log_q, prop.grad_log_q, B, sws, sb, stream));
            FAB_TRY(fabhip_target_log_prob(&a->target, prop.x, prop.log_p, prop.grad_log_p, B, stream));
            FAB_TRY(fabhip_hmc_generic_leap_post(B, D, prop.grad_log_q, prop.grad_log_p, a->cur, a->max_grad, a->epsilons + n,
                                                 a->common_epsilon, gws, gb, stream));
        }
        if (!fold)
            FAB_TRY(gen_hmc_accept(&prop, &cur, B, D, a->cur, a->next, last ? a->log_w : nullptr, a->noise_e + (size_t)n * B, a->mass,
                                   a->epsilons + n, a->common_epsilon, a->target_p_accept, a->tune,
                                   a->p_accept ? a->p_accept + n : nullptr, a->avg_distance, gws, a->n_valid, st));
        start = prop;                                  // the reference continues from the PROPOSAL (hmc.py:133-142)
    }
    return FABHIP_OK;
}

int fabhip_spline_hmc_transition(const fabhip_spline_hmc_args* a, fabhip_stream_t stream) {
    return spline_hmc_transition_impl(a, stream, false);
}

size_t fabhip_spline_ais_workspace_bytes(int32_t dim, int32_t n_layers, int32_t hidden, int64_t B) {
    return carve_spline_ais_ws(nullptr, dim, n_layers, hidden, B).bytes;
}

int fabhip_spline_ais_run(const fabhip_spline_ais_args* a, fabhip_stream_t stream) {
    if (!a || !a->flow.packed || !a->betas || !a->u0 || !a->eps0 || !a->noise_p || !a->noise_e || !a->epsilons ||
        !a->common_epsilon || !a->mass || !a->log_w || !a->n_valid || !a->stats || !a->workspace || a->B < 1 || a->M < 1 ||
        a->n_outer < 1 || a->L < 1)
        return FABHIP_EINVAL;
    FAB_TRY(check_target(&a->target, a->flow.dim));
    FAB_TRY(check_point(a->point, true));
    const int D = a->flow.dim;
    const long B = a->B;
    const SplineAisWs w = carve_spline_ais_ws(a->workspace, D, a->flow.n_layers, a->flow.hidden, B);
    if (a->workspace_bytes < w.bytes) return FABHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    // the spline kernels' own scratch: the transition workspace is free until the first transition
    const size_t sb = fabhip_spline_workspace_bytes(D, a->flow.n_layers, a->flow.hidden, B, 1);
    // 1. chain initialisation: x, log q0 = flow.sample ; point = create_point(x) ; log_w = pi_beta1(point) - log q0
    FAB_TRY(fabhip_spline_sample(&a->flow, a->u0, a->eps0, a->point.x, w.lq0, B, w.trans_ws, sb, stream));
    FAB_TRY(fabhip_spline_log_prob(&a->flow, a->point.x, a->point.log_q, a->point.grad_log_q, B, w.trans_ws, sb, stream));
    FAB_TRY(fabhip_target_log_prob(&a->target, a->point.x, a->point.log_p, a->point.grad_log_p, B, stream));
    fabhip_anneal a1;
    fabhip_anneal_coefs(a->betas[1], a->alpha, a->p_target, &a1);
    launch_spline_init_logw(a->point.log_q, a->point.log_p, w.lq0, a1, a->log_w, a->base_log_w, B, st);
    // 2. "chain init" filter, 3. base ESS
    FAB_TRY(phase_tail(a->point, a->log_w, B, D, nullptr, a->n_valid, w.tmp, w.dest, a->base_log_w, w.lwb, 1.0, a->stats + 0, w.ess_ws,
                       w.ess_bytes, a->base_x, nullptr, a->stats + 6, st));
    // 4. transitions
    for (int j = 1; j <= a->M; ++j) {
        fabhip_spline_hmc_args h;
        h.flow = a->flow; h.target = a->target; h.point = a->point; h.B = B; h.n_valid = a->n_valid;
        fabhip_anneal_coefs(a->betas[j], a->alpha, a->p_target, &h.cur);
        fabhip_anneal_coefs(a->betas[j + 1], a->alpha, a->p_target, &h.next);
        h.log_w = (a->betas[j + 1] != a->betas[j]) ? a->log_w : nullptr;      // ais.py:93
        const size_t nslab = (size_t)(j - 1) * a->n_outer;
        h.noise_p = a->noise_p + nslab * B * D; h.noise_e = a->noise_e + nslab * B;
        h.epsilons = a->epsilons + nslab; h.common_epsilon = a->common_epsilon; h.mass = a->mass;
        h.n_outer = a->n_outer; h.L = a->L; h.max_grad = a->max_grad; h.target_p_accept = a->target_p_accept; h.tune = a->tune;
        h.p_accept = nullptr; h.avg_distance = nullptr;
        if (j == 1) { h.p_accept = a->p_accept_first; h.avg_distance = a->avg_distance_first; }
        else if (j == a->M) { h.p_accept = a->p_accept_last; h.avg_distance = a->avg_distance_last; }
        h.workspace = w.trans_ws; h.workspace_bytes = w.trans_bytes;
        if (j == 1 && spline_leap_fold_supported(&a->flow, B) &&
            hipMemsetAsync(carve_spline_hmc_ws(w.trans_ws, D, a->flow.n_layers, a->flow.hidden, B).ticket, 0, 4, st) != hipSuccess)
            return FABHIP_ELAUNCH;
        FAB_TRY(spline_hmc_transition_impl(&h, stream, true));
    }
    // 5. "chain end" filter, 6. ESS / log Z
    FAB_TRY(phase_tail(a->point, a->log_w, B, D, a->n_valid, a->n_valid + 1, w.tmp, w.dest, nullptr, nullptr, (double)B, a->stats + 3,
                       w.ess_ws, w.ess_bytes, nullptr, nullptr, nullptr, st));
    return check_launch();
}

int fabhip_ais_run(const fabhip_ais_args* a, fabhip_stream_t stream) { return fabhip_ais_run_ext(a, nullptr, stream); }

int fabhip_ais_phase(const fabhip_ais_args* a, int32_t phases, int32_t j_begin, int32_t j_end, float* partials,
                     fabhip_stream_t stream) {
    return fabhip_ais_phase_ext(a, nullptr, phases, j_begin, j_end, partials, stream);
}

int fabhip_ais_run_ext(const fabhip_ais_args* a, const fabhip_ais_ext* ext, fabhip_stream_t stream) {
    if (!a) return FABHIP_EINVAL;
    return fabhip_ais_phase_ext(a, ext, FABHIP_AIS_INIT | FABHIP_AIS_FINISH, 1, a->M, nullptr, stream);
}

int fabhip_ais_phase_ext(const fabhip_ais_args* a, const fabhip_ais_ext* ext, int32_t phases, int32_t j_begin, int32_t j_end,
                         float* partials, fabhip_stream_t stream) {
    AisCall c;
    FAB_TRY(check_ais_call(a, ext, phases, j_begin, j_end, partials, &c.m));
    const bool ws_kept = (phases & (FABHIP_AIS_INIT | FABHIP_AIS_CONTINUE)) != 0;     // the ticket word of this workspace is zero
    c.a = a; c.partials = partials; c.st = (hipStream_t)stream; c.hmc = a->transition == FABHIP_TRANSITION_HMC;
    c.w = carve_ais_ws(a->workspace, a->B, a->flow.dim, a->n_inner, c.m);
    if (a->workspace_bytes < c.w.bytes) return FABHIP_ENOSPC;
    // (the accept kernel leaves its count word zero: one 8-byte fill per call that runs moves)
    if (c.m.mv_on && j_begin <= j_end && hipMemsetAsync(c.w.mv_word, 0, 8, c.st) != hipSuccess) return FABHIP_ELAUNCH;
    c.f = flow_dims_of(a->flow);
    c.tg = make_target_dev(a->target);
    // step-size rule inside the transition kernels (hmc_adapt_last): only where the ticket word is known to be zero (this call's or,
    // with FABHIP_AIS_CONTINUE, an earlier call's init phase zeroed it; every transition kernel leaves it zero)
    c.ticket = (c.hmc && !c.m.mx.on && !partials && option(FABHIP_OPT_ADAPT_FOLD) != 0 && nblk_of(a->B) <= 2048 &&
                (use_r8_tiles(c.f, a->B) || use_r4_tiles(c.f, a->B))) ? c.w.ticket : nullptr;     // (2 nblk floats of LDS scratch)
    // (round 6: a call that runs transitions on a workspace nobody zeroed - the second piece of a call whose INIT piece was its own
    //  fabhip_ais_phase call, fab_torch_amd/ais.py: repeated calls - zeroes the word itself: one 4-byte fill instead of a
    //  k_hmc_adapt launch per transition)
    if (c.ticket && !ws_kept) {
        if (j_begin > j_end) c.ticket = nullptr;
        else if (hipMemsetAsync(c.ticket, 0, 4, c.st) != hipSuccess) return FABHIP_ELAUNCH;
    }
    if (phases & FABHIP_AIS_INIT) FAB_TRY(ais_chain_init(c));
    // 4. transitions: [resampling step,] [moves,] transition j
    for (int j = j_begin; j <= j_end; ++j) {
        fabhip_anneal cj, cn;
        fabhip_anneal_coefs(a->betas[j], a->alpha, a->p_target, &cj);
        fabhip_anneal_coefs(a->betas[j + 1], a->alpha, a->p_target, &cn);
        if (c.m.smc_on) {
            FAB_TRY(ais_resample_step(c, j));
            if (c.m.smc->only_resample) continue;
        }
        if (c.m.mv_on) FAB_TRY(ais_moves_step(c, j, cj));
        FAB_TRY(ais_transition(c, j, cj, cn));
    }
    if (phases & FABHIP_AIS_FINISH) FAB_TRY(ais_finish(c));
    return check_launch();
}

size_t fabhip_flow_move_workspace_bytes(int64_t B, int32_t dim) {
    if (B < 0 || dim < 1) return 0;
    return carve_flow_move_ws(nullptr, B, dim).bytes;
}

int fabhip_flow_move(const fabhip_flow_move_args* a, fabhip_stream_t stream) {
    if (!a || !a->flow.packed || !a->noise_g || !a->noise_h || !a->workspace || a->B < 0 || a->B > 0x3fffffffL) return FABHIP_EINVAL;
    FAB_TRY(check_flow_shape(a->flow.dim, a->flow.n_layers, a->flow.width));
    FAB_TRY(check_target(&a->target, a->flow.dim));
    FAB_TRY(check_point(a->point, false));
    if ((a->point.grad_log_q == nullptr) != (a->point.grad_log_p == nullptr)) return FABHIP_EINVAL;
    if (((size_t)a->workspace & 255) != 0) return FABHIP_EINVAL;
    const FlowMoveWs w = carve_flow_move_ws(a->workspace, a->B, a->flow.dim);
    if (a->workspace_bytes < w.bytes) return FABHIP_ENOSPC;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(w.word, 0, 8, st) != hipSuccess) return FABHIP_ELAUNCH;
    if (a->B == 0) {                   // nothing to move: the outputs of an empty batch
        if (a->p_accept && hipMemsetAsync(a->p_accept, 0, 4, st) != hipSuccess) return FABHIP_ELAUNCH;
        if (a->n_accept && hipMemsetAsync(a->n_accept, 0, 4, st) != hipSuccess) return FABHIP_ELAUNCH;
        return FABHIP_OK;
    }
    return flow_move_impl(a->flow, a->target, a->point, (long)a->B, a->n_valid, a->cur, a->noise_g, a->noise_h, a->p_accept,
                          a->n_accept, w.word, w.prop, st);
}

}  // extern "C"
