"""Cost of the native coupled-quartic target next to ManyWell on the headline shape: RealNVP 10 x (16-320-320-32), D = 32, M = 8,
HMC L = 5, step-size tuning on, 1024 and 2048 chains - the same build, the same session, the settings alternating.

Timing: ms per `sample_and_log_weights` call (wall clock over CALLS calls, REPEATS repeats: median and the min .. max spread) for
  manywell   ManyWell-32, the yardstick (the benchmark's own call),
  phi4       LatticePhi4((4, 8), kappa 0.3, lambda 0.02): the dense 32 x 32 coupling read from global memory per evaluation.
Reported, not asserted (an untrained seeded flow, 1024 chains, AIS target p, tuning off, step 0.1, SEEDS seeds):
  log_Z      plain AIS and SMC mode (tau = 0.5) against the exact normaliser of a correlated Gaussian (c = 0) of the family,
  z2         the weighted share of samples with mean field > 0 on a broken-phase 4 x 4 lattice, plain AIS against SMC mode
             (1/2 is the symmetric answer; 0 or 1 a sampler that sits in one mode).
One JSON line.  PARTS=timing,log_z,z2 in the environment chooses what runs."""
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
PARTS = os.environ.get("PARTS", "timing,log_z,z2").split(",")


def sampler(flow, target, dim, tau=None, p_target=False, tune=True, eps=0.1):
    hmc = fa.HamiltonianMonteCarlo(M, dim, flow.log_prob, target.log_prob, alpha=2.0, p_target=p_target, epsilon=eps, L=L,
                                   eval_mode=not tune).to(DEV)
    return fa.AnnealedImportanceSampler(flow, target.log_prob, hmc, p_target, 2.0, M, resample_threshold=tau)


def time_targets(flow, targets, B):
    """the targets' calls alternating repeat by repeat (drift of the session hits both alike)"""
    ais = {n: sampler(flow, t, D) for n, t in targets.items()}
    for a in ais.values():
        torch.manual_seed(1)
        for _ in range(100):
            a.sample_and_log_weights(B)
    ms = {n: [] for n in ais}
    for _ in range(REPEATS):
        for n, a in ais.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(CALLS):
                a.sample_and_log_weights(B)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / CALLS * 1e3)
    out = {}
    for n, v in ms.items():
        v.sort()
        out[n] = {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1], "ess_ais": ais[n].get_logging_info()["ess_ais"]}
    out["phi4_over_manywell"] = out["phi4"]["ms_median"] / out["manywell"]["ms_median"]
    return out


def small_flow(dim, seed=0):
    torch.manual_seed(seed)
    return fa.make_wrapped_normflow_realnvp(dim, 6, 10, act_norm=False).to(DEV).requires_grad_(False)


def gaussian_instance(dim):
    """a correlated Gaussian of the family: nearest-neighbour ring coupling -0.3, b = 0.5 (P = I + J is positive definite)"""
    J = torch.zeros(dim, dim, dtype=torch.float64)
    i = torch.arange(dim)
    J[i, (i + 1) % dim] = J[(i + 1) % dim, i] = -0.3
    return fa.CoupledQuarticEnergy(torch.linspace(-0.5, 0.5, dim, dtype=torch.float64), torch.full((dim,), 0.5, dtype=torch.float64),
                                   torch.zeros(dim, dtype=torch.float64), J)


def per_seed(flow, target, dim, B, figure):
    out = {}
    for name, tau in (("plain", None), ("smc", 0.5)):
        vals, n_res = [], 0
        for seed in range(SEEDS):
            ais = sampler(flow, target, dim, tau=tau, p_target=True, tune=False)
            torch.manual_seed(100 + seed)
            pt, lw = ais.sample_and_log_weights(B)
            info = ais.get_logging_info()
            vals.append(figure(pt, lw, info))
            n_res += info.get("n_resampled", 0)
        t = torch.tensor(vals, dtype=torch.float64)
        out[name] = {"values": [round(v, 5) for v in vals], "mean": float(t.mean()), "std": float(t.std()), "min": float(t.min()),
                     "max": float(t.max()), "n_resampled": n_res, "of_steps": SEEDS * M}
    return out


def main():
    res = {"lib_srchash": _lib_srchash(), "device": torch.cuda.get_device_name(0), "calls": CALLS, "repeats": REPEATS, "seeds": SEEDS}
    if "timing" in PARTS:
        flow = build_flow_state(0).to(DEV).requires_grad_(False)
        targets = {"manywell": fa.ManyWellEnergy(D), "phi4": fa.LatticePhi4((4, 8), 0.3, 0.02)}
        res["timing_ms_per_call"] = {str(B): time_targets(flow, targets, B) for B in (1024, 2048)}
    if "log_z" in PARTS:
        g = gaussian_instance(16)
        exact = float(g.log_Z)
        res["gaussian_log_Z_error"] = dict(per_seed(small_flow(16), g, 16, 1024, lambda pt, lw, info: info["log_Z"] - exact),
                                           exact_log_Z=exact)
    if "z2" in PARTS:
        lat = fa.LatticePhi4((4, 4), 0.3, 0.02)
        res["z2_positive_share"] = per_seed(small_flow(16), lat, 16, 1024,
                                            lambda pt, lw, info: lat.performance_metrics(pt.x, lw)["positive_share"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
