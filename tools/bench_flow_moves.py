"""Cost and effect of the flow-proposal independence moves (AnnealedImportanceSampler.n_flow_moves) on the same build, in one
session.

cost     ManyWell-32, RealNVP 10 x (16-320-320-32), M = 8, HMC L = 5, step-size tuning on, 1024 and 2048 chains: ms per
         `sample_and_log_weights` call (wall clock over CALLS calls, REPEATS repeats, the settings alternating repeat by repeat:
         median and the min .. max spread) for n_flow_moves = 0 as the benchmark runs it (prefetch on), n_flow_moves = 0 without
         the prefetch (the moves bypass it: the like-for-like baseline), 1 and 2; the per-move increment (ms per call over
         M x n_flow_moves moves); the chain initialisation alone (FABHIP_AIS_INIT through the phase op, HIP events) as the
         yardstick of one move, and one stand-alone fabhip::flow_move (HIP events).
benefit  reported, not asserted - an UNTRAINED seeded flow, SEEDS seeds, identical eps0 for both settings of a seed:
         gmm   the 40-mode GMM in 2-D (RealNVP 4 x W 80, 512 chains, M = 4, Metropolis step 5): final ESS,
         phi4  LatticePhi4((4, 4), kappa 0.3, lambda 0.02), broken phase (RealNVP 6 x W 160, 1024 chains, M = 8, HMC): final ESS
               and the weighted share of samples with mean field > 0 (1/2 is the symmetric answer),
         each with n_flow_moves = 0 and 1 at equal M.
One JSON line.  PARTS=cost,benefit in the environment chooses what runs."""
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
PARTS = os.environ.get("PARTS", "cost,benefit").split(",")


def headline_sampler(flow, target, k):
    hmc = fa.HamiltonianMonteCarlo(M, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.1, L=L).to(DEV)
    return fa.AnnealedImportanceSampler(flow, target.log_prob, hmc, False, 2.0, M, n_flow_moves=k)


def time_settings(flow, target, B):
    """the settings' calls alternating repeat by repeat (drift of the session hits all alike)"""
    settings = {"k0": (0, True), "k0_noprefetch": (0, False), "k1": (1, False), "k2": (2, False)}
    ais = {}
    for name, (k, prefetch) in settings.items():
        ais[name] = headline_sampler(flow, target, k)
        ais[name].prefetch = prefetch
        torch.manual_seed(1)
        for _ in range(100):
            ais[name].sample_and_log_weights(B)
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
        info = ais[n].get_logging_info()
        out[n] = {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1], "ess_ais": info["ess_ais"],
                  "p_accept_first": info.get("flow_move_p_accept_dist0"), "p_accept_last": info.get(f"flow_move_p_accept_dist{M - 1}")}
    base = out["k0_noprefetch"]["ms_median"]
    out["us_per_move_k1"] = (out["k1"]["ms_median"] - base) / M * 1e3
    out["us_per_move_k2"] = (out["k2"]["ms_median"] - base) / (2 * M) * 1e3
    return out


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


def pieces(flow, target, B):
    """the chain initialisation alone and one stand-alone move, back to back on the stream (HIP events: device time + launch gaps)"""
    from fab_torch_amd import _ops
    ais = headline_sampler(flow, target, 0)
    torch.manual_seed(2)
    st = ais.new_phase_state(B)
    init = _event_us(lambda: ais.enqueue_phase(st, 1, 1, 0))
    g, h = torch.randn((B, D), device=DEV), torch.empty(B, device=DEV).exponential_(1.0)
    args = (*flow.native(), *target.native_target(), st["x"], st["lq"], st["lp"], st["gq"], st["gp"], st["n_valid"], 0.5, 2.0, False,
            g, h, _ops.precision_of(flow))
    ops = _ops.load()
    return {"chain_init": init, "flow_move": _event_us(lambda: ops.flow_move(*args))}


def small_flow(dim, layers, nodes, seed=0):
    torch.manual_seed(seed)
    return fa.make_wrapped_normflow_realnvp(dim, layers, nodes, act_norm=False).to(DEV).requires_grad_(False)


def benefit(make, B, dim, figure):
    """per seed: the same eps0 for n_flow_moves = 0 and 1; the transition noise is each call's own"""
    out = {}
    for k in (0, 1):
        vals = []
        for seed in range(SEEDS):
            ais = make(k)
            eps0 = torch.randn((B, dim), generator=torch.Generator().manual_seed(500 + seed)).to(DEV)
            torch.manual_seed(100 + seed)
            pt, lw = ais.sample_and_log_weights(B, eps0=eps0)
            info = ais.get_logging_info()
            vals.append(figure(pt, lw, info))
        keys = vals[0].keys()
        out[f"k{k}"] = {key: {"values": [round(v[key], 5) for v in vals],
                              "mean": float(torch.tensor([v[key] for v in vals], dtype=torch.float64).mean()),
                              "std": float(torch.tensor([v[key] for v in vals], dtype=torch.float64).std())} for key in keys}
    return out


def main():
    res = {"lib_srchash": _lib_srchash()[:12], "device": torch.cuda.get_device_name(0), "calls": CALLS, "repeats": REPEATS,
           "seeds": SEEDS}
    if "cost" in PARTS:
        flow = build_flow_state(0).to(DEV).requires_grad_(False)
        target = fa.ManyWellEnergy(D)
        res["cost"] = {f"B{B}": {**time_settings(flow, target, B), **pieces(flow, target, B)} for B in (1024, 2048)}
    if "benefit" in PARTS:
        torch.manual_seed(0)
        gmm = fa.GMM(2, 40, 40.0, 1.0)
        gflow = small_flow(2, 4, 40)

        def make_gmm(k):
            op = fa.Metropolis(4, 2, gflow.log_prob, gmm.log_prob, n_updates=1, alpha=2.0, p_target=False, max_step_size=5.0,
                               min_step_size=5.0, adjust_step_size=False).to(DEV)
            return fa.AnnealedImportanceSampler(gflow, gmm.log_prob, op, False, 2.0, 4, n_flow_moves=k)
        res["gmm40"] = benefit(make_gmm, 512, 2, lambda pt, lw, info: {"ess_ais": info["ess_ais"],
                                                                       "p_accept_last": info.get("flow_move_p_accept_dist3", 0.0)})
        lat = fa.LatticePhi4((4, 4), 0.3, 0.02)
        lflow = small_flow(16, 6, 10)

        def make_phi4(k):
            op = fa.HamiltonianMonteCarlo(M, 16, lflow.log_prob, lat.log_prob, alpha=2.0, p_target=True, epsilon=0.1, L=L,
                                          eval_mode=True).to(DEV)
            return fa.AnnealedImportanceSampler(lflow, lat.log_prob, op, True, 2.0, M, n_flow_moves=k)
        res["phi4_4x4_broken"] = benefit(make_phi4, 1024, 16, lambda pt, lw, info: {
            "ess_ais": info["ess_ais"], "positive_share": lat.performance_metrics(pt.x, lw)["positive_share"],
            "p_accept_last": info.get(f"flow_move_p_accept_dist{M - 1}", 0.0)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
