"""Cost of the native coupled-quartic and coupled-rotor targets next to ManyWell on the headline shape: RealNVP 10 x (16-320-320-32), D = 32, M = 8,
HMC L = 5, step-size tuning on, 1024 and 2048 chains - the same build, the same session, the settings alternating.

Timing: ms per `sample_and_log_weights` call (wall clock over CALLS calls, REPEATS repeats: median and the min .. max spread) for
  manywell   ManyWell-32, the yardstick (the benchmark's own call),
  phi4       LatticePhi4((4, 8), kappa 0.3, lambda 0.02): the dense 32 x 32 coupling read from global memory per evaluation.
Reported, not asserted (an untrained seeded flow, 1024 chains, AIS target p, tuning off, step 0.1, SEEDS seeds):
  log_Z      plain AIS and SMC mode (tau = 0.5) against the exact normaliser of a correlated Gaussian (c = 0) of the family,
  z2         the weighted share of samples with mean field > 0 on a broken-phase 4 x 4 lattice, plain AIS against SMC mode
             (1/2 is the symmetric answer; 0 or 1 a sampler that sits in one mode).
The coupled-rotor target (CoupledRotorEnergy / LatticeXY), same session:
  xy         LatticeXY((4, 8), 0.5, field 0.2) under the same RealNVP call (timing; four neighbours a site),
  spline     the spline-flow call on the 60-D shape of BASELINE cfg 5 (12 layers, hidden 256, 12 circular coordinates, M = 20,
             10 leapfrogs, 4096 chains): ManyWell-60 against `torsion_stand_in` - the 12 circular coordinates as coupled torsions
             (three Fourier harmonics, couplings to the next and the next-but-one torsion) on the flow's own torus, the other 48
             as harmonic line sites,
  vm_log_z   log_Z error on an independent von Mises product (exact constant),
  xy_mag     weighted |m| of LatticeXY((4, 4)) at a low (0.2) and a high (1.5) coupling - both with plain AIS (target p) from a
             spline flow on the target's torus: a periodic density has no finite integral against a flow on the line, and the
             fused spline call has no SMC mode,
  xy_mag_smc the same |m| (a ratio of weighted sums: it needs no normaliser) from the RealNVP base of `z2`, where SMC mode
             exists: plain AIS against SMC mode (tau = 0.5).
One JSON line.  PARTS in the environment chooses what runs: timing,log_z,z2 by default; spline, vm_log_z, xy_mag and xy_mag_smc
(the 60-D spline call is long) only when named."""
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
    for n in ais:
        if n != "manywell":
            out[f"{n}_over_manywell"] = out[n]["ms_median"] / out["manywell"]["ms_median"]
    return out


SPLINE_D, SPLINE_M, SPLINE_LF, SPLINE_B = 60, 20, 10, 4096
SPLINE_CIRC = (3, 7, 8, 12, 20, 21, 22, 30, 41, 45, 52, 59)


def torsion_stand_in(flow):
    """the cfg-5-shaped rotor target on the torus of `flow`: its circular coordinates as a chain of coupled torsions (Fourier
    rows of three harmonics; couplings 0.5 to the next torsion and 0.2 to the next but one), every other coordinate harmonic"""
    circ = torch.nonzero(flow._circ.cpu()).flatten().tolist()
    dim = flow.dim
    A, Bc = torch.zeros(3, dim, dtype=torch.float64), torch.zeros(3, dim, dtype=torch.float64)
    K = torch.zeros(dim, dim, dtype=torch.float64)
    for n, j in enumerate(circ):
        A[:, j] = torch.tensor([1.0, 0.3, 0.2], dtype=torch.float64) * (1.0 if n % 2 == 0 else -0.8)
        Bc[:, j] = torch.tensor([0.5, -0.2, 0.1], dtype=torch.float64)
        for step, kap in ((1, 0.5), (2, 0.2)):
            if n + step < len(circ):
                K[j, circ[n + step]] = K[circ[n + step], j] = kap
    line = torch.ones(dim, dtype=torch.float64)
    line[circ] = 0.0
    return fa.CoupledRotorEnergy.for_flow(flow, A, Bc, K, line_quadratic=0.5 * line)


def time_spline_targets():
    import math
    tb = torch.full((SPLINE_D,), 5.0)
    tb[list(SPLINE_CIRC)] = math.pi
    torch.manual_seed(0)
    flow = fa.make_wrapped_normflow_spline(SPLINE_D, 12, 256, SPLINE_CIRC, tb).to(DEV).requires_grad_(False)
    with torch.no_grad():
        for p in flow.parameters():
            if p.dim() == 2 and p.shape[0] % 25 == 0:
                p.add_(0.02 * torch.randn_like(p))
    targets = {"manywell": fa.ManyWellEnergy(SPLINE_D), "torsions": torsion_stand_in(flow)}
    ais = {}
    for n, t in targets.items():
        hmc = fa.HamiltonianMonteCarlo(SPLINE_M, SPLINE_D, flow.log_prob, t.log_prob, alpha=2.0, p_target=False, epsilon=0.1,
                                       L=SPLINE_LF).to(DEV)
        ais[n] = fa.AnnealedImportanceSampler(flow, t.log_prob, hmc, False, 2.0, SPLINE_M)
        for _ in range(2):
            ais[n].sample_and_log_weights(SPLINE_B)
    calls = max(2, CALLS // 40)
    ms = {n: [] for n in ais}
    for _ in range(REPEATS):
        for n, a in ais.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(calls):
                a.sample_and_log_weights(SPLINE_B)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) / calls * 1e3)
    out = {"calls": calls, "n_neighbours": targets["torsions"].n_neighbours}
    for n, v in ms.items():
        v.sort()
        out[n] = {"ms_median": v[len(v) // 2], "ms_min": v[0], "ms_max": v[-1]}
    out["torsions_over_manywell"] = out["torsions"]["ms_median"] / out["manywell"]["ms_median"]
    return out


def torus_flow(period, seed=0):
    """a spline flow with every coordinate circular on the torus of the given periods: the base a periodic target's normaliser
    is defined against (a flow on the line meets a periodic density with an infinite integral).  The fused spline call has no
    SMC mode, so the rotor figures are plain AIS."""
    dim = period.shape[0]
    torch.manual_seed(seed)
    flow = fa.make_wrapped_normflow_spline(dim, 4, 256, tuple(range(dim)), 0.5 * period.float()).to(DEV).requires_grad_(False)
    with torch.no_grad():
        for p in flow.parameters():
            if p.dim() == 2 and p.shape[0] % 25 == 0:
                p.add_(0.02 * torch.randn_like(p))
    return flow


PLAIN = (("plain", None),)


def von_mises_instance(dim):
    """independent single-harmonic rotors of distinct periods and concentrations: log_Z = sum_j log(P_j I0(kappa_j)) exactly"""
    j = torch.arange(dim, dtype=torch.float64)
    return fa.CoupledRotorEnergy(3.0 + 0.25 * j, 1.5 * torch.cos(0.7 * j), 1.5 * torch.sin(0.7 * j), torch.zeros(dim, dim))


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


def per_seed(flow, target, dim, B, figure, modes=(("plain", None), ("smc", 0.5)), p_target=True):
    out = {}
    for name, tau in modes:
        vals, n_res = [], 0
        for seed in range(SEEDS):
            ais = sampler(flow, target, dim, tau=tau, p_target=p_target, tune=False)
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
        targets = {"manywell": fa.ManyWellEnergy(D), "phi4": fa.LatticePhi4((4, 8), 0.3, 0.02),
                   "xy": fa.LatticeXY((4, 8), 0.5, field=0.2)}
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
    if "spline" in PARTS:
        res["spline_timing_ms_per_call"] = time_spline_targets()
    if "vm_log_z" in PARTS:
        vm = von_mises_instance(16)
        exact = float(vm.log_Z)
        res["von_mises_log_Z_error"] = dict(per_seed(torus_flow(vm._P64), vm, 16, 1024, lambda pt, lw, info: info["log_Z"] - exact,
                                                     PLAIN), exact_log_Z=exact)
    if "xy_mag" in PARTS:
        res["xy_abs_magnetisation"] = {}
        for coupling in (0.2, 1.5):
            lat = fa.LatticeXY((4, 4), coupling)
            res["xy_abs_magnetisation"][str(coupling)] = per_seed(
                torus_flow(lat._P64), lat, 16, 1024, lambda pt, lw, info: lat.performance_metrics(pt.x, lw)["abs_magnetisation"],
                PLAIN)
    if "xy_mag_smc" in PARTS:
        res["xy_abs_magnetisation_realnvp_base"] = {}
        for coupling in (0.2, 1.5):
            lat = fa.LatticeXY((4, 4), coupling)
            res["xy_abs_magnetisation_realnvp_base"][str(coupling)] = per_seed(
                small_flow(16), lat, 16, 1024, lambda pt, lw, info: lat.performance_metrics(pt.x, lw)["abs_magnetisation"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
