"""Cost of the defensive-mixture base distribution (fab_torch_amd.DefensiveMixtureDistribution) on the headline workload:
ManyWell-32, RealNVP 10 x (16-320-320-32), M = 8, HMC L = 5, step-size tuning on, 1024 / 2048 / 4096 chains.

ms per `sample_and_log_weights` call (wall clock over CALLS calls, REPEATS repeats: median and the min .. max spread) for
  plain            the plain call as bench.py runs it (its own tile choice: 4-chain tiles up to 1152 chains, 8-chain tiles up to
                   8 per compute unit; prefetch of repeated calls on),
  plain/16         the plain one-op call with the 16-chain tile forced (FABHIP_OPT_TILE_SHAPE = 16) and the prefetch off: the
                   like-for-like baseline of the mixture, which runs on 16-chain tiles at every batch size and bypasses the prefetch,
  mixture          the same sampler over DefensiveMixtureDistribution(flow) at its default parameters.
`plain` next to `plain/16` is the price of leaving the 4- / 8-chain tiles, `mixture` next to `plain/16` the price of the epilogue.

With WHAT_IT_BUYS=1 also the recipe of tools/bench_trainer.py from a fresh flow (float32), ITERS iterations (default 300) with the
plain flow and with the mixture at default parameters, same seeds: first iteration with a non-finite loss, number of skipped
minibatch steps, largest |x| that entered the buffer, final ess_ais.  One JSON line."""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import fab_torch_amd as fa
from fab_torch_amd import _ops
from bench import build_flow_state, _lib_srchash      # the bench's seeded headline flow

DEV = "cuda"
D, M, L = 32, 8, 5
CALLS, REPEATS = int(os.environ.get("CALLS", 100)), int(os.environ.get("REPEATS", 5))


def sampler(mixture: bool):
    flow = build_flow_state(0).to(DEV).requires_grad_(False)
    base = fa.DefensiveMixtureDistribution(flow).to(DEV).requires_grad_(False) if mixture else flow
    target = fa.ManyWellEnergy(D)
    hmc = fa.HamiltonianMonteCarlo(M, D, base.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.1, L=L).to(DEV)
    return fa.AnnealedImportanceSampler(base, target.log_prob, hmc, False, 2.0, M)


def time_setting(B, mixture, prefetch, tile):
    ais = sampler(mixture)
    ais.prefetch = prefetch
    torch.manual_seed(1)
    with _ops.option(_ops.OPT_TILE_SHAPE, tile):
        for _ in range(50):
            ais.sample_and_log_weights(B)
        ms = []
        for _ in range(REPEATS):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(CALLS):
                ais.sample_and_log_weights(B)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / CALLS * 1e3)
    ms.sort()
    return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "ess_ais": ais.get_logging_info()["ess_ais"]}


def what_it_buys(mixture: bool, iters: int):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import bench_trainer as bt
    from fab_torch_amd.buffer import PrioritisedReplayBuffer
    torch.manual_seed(0)
    flow = fa.make_wrapped_normflow_realnvp(bt.D, n_flow_layers=bt.K_LAYERS, layer_nodes_per_dim=bt.NODES, act_norm=False).to(DEV)
    base = fa.DefensiveMixtureDistribution(flow).to(DEV) if mixture else flow
    target = fa.ManyWellEnergy(bt.D)
    hmc = fa.HamiltonianMonteCarlo(bt.M, bt.D, base.log_prob, target.log_prob, alpha=bt.ALPHA, p_target=False, epsilon=0.2,
                                   n_outer=1, L=bt.L).to(DEV)
    model = fa.FABModel(base, target, bt.M, alpha=bt.ALPHA, transition_operator=hmc, loss_type="fab_alpha_div")
    ais = model.annealed_importance_sampler
    # (the mixture trains through the autograd branch: torch Adam for both runs, so that they differ in the base distribution only)
    opt = torch.optim.Adam(model.parameters(), lr=bt.LR)
    seen = {"max_abs_x": 0.0}

    def track(x):
        seen["max_abs_x"] = max(seen["max_abs_x"], float(x.abs().max()))

    def init_sampler():
        pt, lw = ais.sample_and_log_weights(bt.BATCH, logging=False)
        track(pt.x)
        return pt.x, lw, pt.log_q
    buf = PrioritisedReplayBuffer(bt.D, bt.BUFFER, bt.MIN_BUFFER, init_sampler, device=DEV)
    add = buf.add

    def add_tracked(x, log_w, log_q):
        track(x)
        return add(x, log_w, log_q)
    buf.add = add_tracked
    trainer = fa.PrioritisedBufferTrainer(model, opt, buf, alpha=bt.ALPHA, n_batches_buffer_sampling=bt.NB,
                                          max_gradient_norm=bt.MAX_GRAD_NORM, w_adjust_max_clip=None)
    first_bad, skipped, info = None, 0, {}
    for i in range(iters):
        try:
            info = trainer.step(i + 1, bt.BATCH)
        except Exception as e:                         # noqa: BLE001 - "No valid points": the run has left the finite range for good
            return {"iterations": i, "first_nonfinite_loss_iteration": first_bad if first_bad is not None else i + 1,
                    "skipped_minibatch_steps": skipped, "max_abs_x_into_buffer": seen["max_abs_x"], "final_ess_ais": None,
                    "stopped": str(e)[:120]}
        stats = trainer.minibatch_stats()
        bad = sum(1 for s in stats if not math.isfinite(s["loss"]))
        skipped += bad
        if bad and first_bad is None:
            first_bad = i + 1
    return {"iterations": iters, "first_nonfinite_loss_iteration": first_bad, "skipped_minibatch_steps": skipped,
            "max_abs_x_into_buffer": seen["max_abs_x"], "final_ess_ais": info.get("ess_ais")}


if __name__ == "__main__":
    out = {"workload": f"ManyWell-{D}, RealNVP 10x(16-320-320-32)+InvAffine, M = {M}, HMC L = {L}, tuning on", "calls": CALLS,
           "repeats": REPEATS, "lib": _lib_srchash(), "ms_per_call": {}}
    for B in (1024, 2048, 4096):
        out["ms_per_call"][str(B)] = {"plain": time_setting(B, False, True, 0), "plain/16": time_setting(B, False, False, 16),
                                      "mixture": time_setting(B, True, False, 0)}
    if os.environ.get("WHAT_IT_BUYS") == "1":
        iters = int(os.environ.get("ITERS", 300))
        out["what_it_buys"] = {"plain": what_it_buys(False, iters), "mixture": what_it_buys(True, iters)}
    print(json.dumps(out))
