"""Cost and effect of the SMC mode (AnnealedImportanceSampler.resample_threshold) on the headline workload: ManyWell-32, RealNVP
10 x (16-320-320-32), M = 8, HMC L = 5, step-size tuning on, 1024 and 2048 chains.

Timing: ms per `sample_and_log_weights` call (wall clock over CALLS calls, REPEATS repeats: median and the min .. max spread) for
  off            the plain call as the benchmark runs it (prefetch of repeated calls on),
  off/noprefetch the plain one-op call (the mode bypasses the prefetch: this is the like-for-like baseline of the next two),
  tau=0          the decision runs before every transition and never fires,
  tau=1.5        it fires every time (gather + copy-back move the whole point).
log Z: error of the call's log_Z against the target's exact normaliser (AIS target p, tuning off, step 0.1) over SEEDS seeds for
off and tau = 0.5, with the untrained seeded flow of the benchmark.
Resampling step alone (HIP events around CALLS steps, REPEATS repeats, us per step): the sharded step - smc_shard_pack +
smc_shard_resample on an emulated gathered buffer of 8 ranks x 2048 chains (the collective itself is NOT in it) - next to the
single-device step (decision + gather + copy-back, ais_phase_smc with only_resample) at 2048 and at 16384 chains, each firing
(tau = 1.5) and not firing (tau = 0).  One JSON line.

METHOD=systematic|stratified in the environment chooses the sampler's `resample_method` for all of it (the sharded step is
systematic only and is left out for stratified).  QUICK_TAU=0.5: only the call's timing at that threshold, 1024 and 2048 chains,
for BOTH methods alternating - the comparison of the two schemes."""
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
METHOD = os.environ.get("METHOD", "systematic")
flow = build_flow_state(0).to(DEV).requires_grad_(False)
target = fa.ManyWellEnergy(D)


def sampler(tau, p_target=False, tune=True, eps=0.1, method=None):
    hmc = fa.HamiltonianMonteCarlo(M, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=p_target, epsilon=eps, L=L,
                                   eval_mode=not tune).to(DEV)
    return fa.AnnealedImportanceSampler(flow, target.log_prob, hmc, p_target, 2.0, M, resample_threshold=tau,
                                        resample_method=METHOD if method is None else method)


def time_setting(B, tau, prefetch, method=None):
    ais = sampler(tau, method=method)
    ais.prefetch = prefetch
    torch.manual_seed(1)
    for _ in range(100):
        ais.sample_and_log_weights(B)
    ms = []
    for _ in range(REPEATS):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(CALLS):
            ais.sample_and_log_weights(B)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / CALLS * 1e3)
    ms.sort()
    info = ais.get_logging_info()
    return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "n_resampled": info.get("n_resampled"),
            "ess_ais": info["ess_ais"]}


def log_z_errors(B, tau):
    errs, n_res = [], 0
    for seed in range(SEEDS):
        ais = sampler(tau, p_target=True, tune=False)
        torch.manual_seed(100 + seed)
        ais.sample_and_log_weights(B)
        info = ais.get_logging_info()
        errs.append(info["log_Z"] - float(target.log_Z))
        n_res += info.get("n_resampled", 0)
    t = torch.tensor(errs, dtype=torch.float64)
    return {"mean": float(t.mean()), "std": float(t.std()), "min": float(t.min()), "max": float(t.max()), "n_resampled": n_res,
            "of_steps": SEEDS * M}


def _event_us(fn):
    """us per call of `fn`: CALLS calls between two HIP events, REPEATS repeats (median, min, max) after a warm-up."""
    for _ in range(100):
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


def _phase_state(B, tau):
    """A sampler's state after FABHIP_AIS_INIT, stepped through the phase op (the sharded backend's own state tensors)."""
    from fab_torch_amd import parallel
    ais = sampler(tau, tune=False)
    be = parallel.HipShardBackend(ais)
    torch.manual_seed(2)
    return ais, be, be.begin(B)


def single_device_step(B, tau):
    from fab_torch_amd import _ops
    ais, be, st = _phase_state(B, tau)
    from fab_torch_amd.ais import operator_slots
    nr = torch.rand(M, dtype=torch.float64, device=DEV)
    args = (*be._common(st), 0, 1, 1, st["eps0"], st["noise_a"], st["noise_b"], *operator_slots(be.op)[1][:7], False, st["x"],
            st["lq"], st["lp"], st["gq"], st["gp"], st["log_w"], st["n_valid"], st["stats"], None, None, None, None, None, None,
            None, _ops.precision_of(flow), float(tau), nr, True, None, None, None, None,
            fa.ais.RESAMPLE_METHODS[METHOD])
    return _event_us(lambda: be.ops.ais_phase_smc(*args))


def sharded_step(R, b, tau):
    """pack + resample of rank 0 on a gathered buffer made of R copies of its own send buffer (with their own log-weights)."""
    ais, be, st = _phase_state(b, tau)
    u = torch.rand(1, dtype=torch.float64, device=DEV)
    gathered = be.pack(st).repeat(R, 1)
    gathered.view(R, b + 1, -1)[:, :b, 3 * D + 2] += torch.randn(R, b, device=DEV)

    def step():
        be.pack(st)
        be.resample(st, 1, gathered, R, 0, u)
    return _event_us(step)


out = {"config": f"ManyWell-{D}, RealNVP 10x(16-320-320-32), M={M}, HMC L={L}", "lib_srchash": _lib_srchash()[:12],
       "calls": CALLS, "repeats": REPEATS, "method": METHOD}
if os.environ.get("QUICK_TAU"):
    tau = float(os.environ["QUICK_TAU"])
    for B in (1024, 2048):
        out[f"B{B}"] = {f"{m}_{i}": time_setting(B, tau, False, method=m) for i in range(2) for m in ("systematic", "stratified")}
    print(json.dumps(out))
    sys.exit(0)
for B in (1024, 2048):
    row = {"off": time_setting(B, None, True), "off_noprefetch": time_setting(B, None, False),
           "tau_0": time_setting(B, 0.0, False), "tau_1.5": time_setting(B, 1.5, False)}
    base = row["off_noprefetch"]["ms_median"]
    row["us_per_transition_tau_0"] = (row["tau_0"]["ms_median"] - base) / M * 1e3
    row["us_per_transition_tau_1.5"] = (row["tau_1.5"]["ms_median"] - base) / M * 1e3
    out[f"B{B}"] = row
out["log_Z_error_B1024"] = {"off": log_z_errors(1024, None), "tau_0.5": log_z_errors(1024, 0.5)}
out["resampling_step_us"] = {
    f"tau_{tau}": {**({"sharded_R8_b2048": sharded_step(8, 2048, tau)} if METHOD == "systematic" else {}),
                   "single_B2048": single_device_step(2048, tau),
                   "single_B16384": single_device_step(16384, tau)} for tau in (1.5, 0.0)}
out["resampling_step_us"]["state_payload_bytes_per_rank"] = {"sent": (2048 + 1) * (3 * D + 4) * 4, "received": 8 * (2048 + 1) * (3 * D + 4) * 4}
print(json.dumps(out))
