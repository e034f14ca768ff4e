"""Cost and effect of adaptive annealing schedules (AnnealedImportanceSampler(distribution_spacing_type="adaptive")) on the headline
workload: ManyWell-32, RealNVP 10 x (16-320-320-32), M = 8, HMC L = 5, step-size tuning on, 1024 and 2048 chains.

Timing: ms per `sample_and_log_weights` call (wall clock over CALLS calls, REPEATS repeats: median and the min .. max spread) for
  linear            the plain fused call as the benchmark runs it (prefetch of repeated calls on),
  linear/noprefetch the plain one-op call,
  linear/stepped    the linear schedule through the stepped driver (`run(force_betas=B_space)`: the decisions run, their answers
                    are not used) - what the M host round trips and the M + 1 single-workgroup launches cost on the same work,
  rho=0.7           the adaptive schedule,
  rho=0.7,tau=0.5   the adaptive schedule with the SMC mode's resampling step in front of every transition.
log Z: error of the call's log_Z against the target's exact normaliser (AIS target p, tuning off, step 0.1) over SEEDS seeds for
linear, rho = 0.7 and rho = 0.5, with the untrained seeded flow of the benchmark; the schedules of the first seed.
Decision kernels alone (HIP events around CALLS launches, REPEATS repeats, us per launch): fabhip::next_beta on the weights of a
chain initialisation - interior answer, 26 evaluations - next to fabhip::smc_decide on the same weights.  KERNELS_ONLY=1 runs only
these launches (for a kernel-trace run of its own).  One JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fab_torch_amd as fa
from bench import build_flow_state, _lib_srchash      # the bench's seeded headline flow

DEV = "cuda"
D, M, L = 32, 8, 5
CALLS, REPEATS, SEEDS = int(os.environ.get("CALLS", 200)), int(os.environ.get("REPEATS", 5)), int(os.environ.get("SEEDS", 8))
flow = build_flow_state(0).to(DEV).requires_grad_(False)
target = fa.ManyWellEnergy(D)


def sampler(spacing="linear", rho=0.7, tau=None, p_target=False, tune=True, eps=0.1):
    hmc = fa.HamiltonianMonteCarlo(M, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=p_target, epsilon=eps, L=L,
                                   eval_mode=not tune).to(DEV)
    return fa.AnnealedImportanceSampler(flow, target.log_prob, hmc, p_target, 2.0, M, distribution_spacing_type=spacing,
                                        ess_decay=rho, resample_threshold=tau)


def time_setting(B, spacing="linear", tau=None, prefetch=True, stepped=False):
    ais = sampler(spacing, tau=tau)
    ais.prefetch = prefetch
    torch.manual_seed(1)
    if stepped:
        forced = ais.B_space.clone()

        def call():
            _, _, n_valid, stats, _, _ = ais.run(B, force_betas=forced)
            fa._ops.read_counts_and_stats(n_valid, stats)                 # the call's own 72-byte read
    else:
        def call():
            ais.sample_and_log_weights(B)
    for _ in range(50):
        call()
    ms = []
    for _ in range(REPEATS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / CALLS * 1e3)
    ms.sort()
    out = {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1]}
    if ais.adaptive:
        out["last_betas"] = [round(b, 5) for b in ais.last_betas.tolist()]
        out["decisions_last_call"] = len(ais.last_adaptive)
    if not stepped:
        info = ais.get_logging_info()
        out.update({k: info[k] for k in ("ess_ais", "n_resampled", "n_steps_to_beta_one", "n_bisect_floor") if k in info})
    return out


def log_z_errors(B, spacing, rho=0.7, tau=None):
    errs, first = [], None
    for seed in range(SEEDS):
        ais = sampler(spacing, rho=rho, tau=tau, p_target=True, tune=False)
        torch.manual_seed(100 + seed)
        ais.sample_and_log_weights(B)
        errs.append(ais.get_logging_info()["log_Z"] - float(target.log_Z))
        if first is None and ais.adaptive:
            first = [round(b, 5) for b in ais.last_betas.tolist()]
    t = torch.tensor(errs, dtype=torch.float64)
    return {"mean": float(t.mean()), "std": float(t.std()), "min": float(t.min()), "max": float(t.max()), "betas_seed0": first}


def _event_us(fn):
    for _ in range(50):
        fn()
    us = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record(); e1.synchronize()
        us.append(e0.elapsed_time(e1) / CALLS * 1e3)
    us.sort()
    return {"us_median": us[len(us) // 2], "us_min": us[0], "us_max": us[-1]}


def decision_kernels(B):
    """The two decision kernels on the weights a chain initialisation at beta = 0 leaves (log_w = log q - log q0, d = log p - log q)."""
    ops = fa._ops.load()
    ais = sampler("adaptive", tune=False)
    torch.manual_seed(2)
    st = ais.new_phase_state(B)
    ais.enqueue_phase(st, 1, 1, 0)
    lw, lq, lp, nv = st["log_w"], st["lq"], st["lp"], st["n_valid"]
    u = torch.rand(1, dtype=torch.float64, device=DEV)
    out4 = ops.next_beta(lw, lq, lp, nv, 0.0, 2.0, False, 0.7).tolist()
    return {"next_beta_out4": out4,
            "next_beta": _event_us(lambda: ops.next_beta(lw, lq, lp, nv, 0.0, 2.0, False, 0.7)),
            "smc_decide": _event_us(lambda: ops.smc_decide(lw, 0.0, u))}


out = {"config": f"ManyWell-{D}, RealNVP 10x(16-320-320-32), M={M}, HMC L={L}", "lib_srchash": _lib_srchash()[:12],
       "calls": CALLS, "repeats": REPEATS}
if os.environ.get("KERNELS_ONLY"):
    out["decision_kernels_us"] = {f"B{B}": decision_kernels(B) for B in (1024, 2048)}
    print(json.dumps(out))
    sys.exit(0)
for B in (1024, 2048):
    out[f"B{B}"] = {"linear": time_setting(B), "linear_noprefetch": time_setting(B, prefetch=False),
                    "linear_stepped": time_setting(B, "adaptive", stepped=True),
                    "rho_0.7": time_setting(B, "adaptive"), "rho_0.7_tau_0.5": time_setting(B, "adaptive", tau=0.5)}
out["log_Z_error_B1024"] = {"linear": log_z_errors(1024, "linear"), "rho_0.7": log_z_errors(1024, "adaptive", 0.7),
                            "rho_0.5": log_z_errors(1024, "adaptive", 0.5),
                            "linear_tau_0.5": log_z_errors(1024, "linear", tau=0.5),
                            "rho_0.7_tau_0.5": log_z_errors(1024, "adaptive", 0.7, tau=0.5)}
out["decision_kernels_us"] = {f"B{B}": decision_kernels(B) for B in (1024, 2048)}
print(json.dumps(out))
