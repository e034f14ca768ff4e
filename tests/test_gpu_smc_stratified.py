"""SMC mode with stratified ancestors (resample_method="stratified"; include/fabhip.h: fabhip_smc_args.method) on the GPU against
its specification (tests/resample_stratified_spec.py: decide - the decision of tests/smc_spec.py with the stratified resampler's
ancestors).  Like tests/test_gpu_smc.py, whose inputs and helpers this file uses, every decision is teacher-forced: the device's
own `log_w_pre[j]` goes into the spec, whose decision and ancestors must EQUAL the device's.  The decision is integer sums and
one float64 expression of IEEE operations on both sides, so it is compared as it is, however close ess comes to tau."""
import numpy as np
import pytest
import torch

import resample_stratified_spec as sspec
import smc_spec
import test_gpu_smc as base

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops, parallel            # noqa: E402

DEV = "cuda"
D, M = base.D, base.M
TAU_MID = base.TAU_MID
STRATIFIED = 1                                     # FABHIP_SMC_STRATIFIED


def samplers(hmc=True, tau=None, eval_mode=True, method="stratified"):
    nf, hf, target, op, ais = base.samplers(hmc=hmc, tau=tau, eval_mode=eval_mode)
    ais.resample_method = method
    return nf, hf, target, op, ais


class Phased(base.Phased):
    def smc(self, phases, j0, j1, tau, only_resample=False, method=STRATIFIED):
        _ops.load().ais_phase_smc(*self._common(phases, j0, j1), tau, self.nr if tau is not None else None, bool(only_resample),
                                  self.resampled, self.ess, self.ancestors, self.log_w_pre, method)


def check_decision(log_w_pre, n0, tau, u, anc_dev, resampled_dev, ess_dev, tag):
    """The device's decision against the stratified spec fed with the weights the device saw."""
    lw = log_w_pre[:n0].cpu().numpy()
    d = sspec.decide(lw, tau, float(u))
    print(f"{tag}: ess {d.ess:.5f} tau {tau} resampled {d.resampled}")
    assert bool(resampled_dev) == d.resampled, f"{tag}: decision differs (spec ess {d.ess}, device ess {float(ess_dev)})"
    assert abs(float(ess_dev) - d.ess) <= 1e-6 * d.ess, f"{tag}: ess {float(ess_dev)} vs {d.ess}"
    anc = anc_dev.cpu().numpy().astype(np.int64)
    assert np.array_equal(anc[:n0], d.ancestors), f"{tag}: {int((anc[:n0] != d.ancestors).sum())} ancestors differ"
    assert np.array_equal(anc[n0:], np.arange(n0, anc.shape[0])), f"{tag}: rows beyond n0 must map to themselves"
    return d


@pytest.mark.parametrize("hmc", [True, False])
@pytest.mark.parametrize("tau", [1.5, TAU_MID])
@pytest.mark.parametrize("shape,B,kill", [(16, 100, ()), (8, 100, ()), (4, 101, ()), (4, 100, (3, 40)), (8, 99, (0,)), (16, 64, (63,))])
def test_decisions_gather_and_common_log_weight_equal_the_spec(shape, B, kill, tau, hmc):
    """Phase by phase on every tile shape, with rows the chain-init filter killed (n0 < B): decision, ess and ancestors equal the
    spec, the point is the gathered rows, every live log_w is the common log-weight where the step fired and untouched else."""
    eps0, na, nb, nr = base.inputs(B, seed=2, hmc=hmc, kill=kill)
    _, _, _, _, ais = samplers(hmc=hmc, tau=tau)
    with _ops.option(_ops.OPT_TILE_SHAPE, shape):
        p = Phased(ais, B, eps0, na, nb, nr)
        p.smc(1, 1, 0, tau)                              # FABHIP_AIS_INIT
        n0 = int(p.n_valid[0])
        assert n0 == B - len(kill)
        fired = 0
        for j in range(1, M + 1):
            before, lw_before = p.point(), p.log_w.clone()
            p.smc(0, j, j, tau, only_resample=True)
            assert torch.equal(p.log_w_pre[j - 1][:n0], lw_before[:n0])
            d = check_decision(p.log_w_pre[j - 1], n0, tau, nr[j - 1], p.ancestors[j - 1], p.resampled[j - 1], p.ess[j - 1],
                               f"transition {j}")
            fired += d.resampled
            idx = p.ancestors[j - 1].long()
            for name, u, v in zip(("x", "log_q", "log_p", "grad_log_q", "grad_log_p"), before, p.point()):
                if u is None:
                    continue
                assert torch.equal(v[:n0], u[idx[:n0]]), f"transition {j}: {name} is not the gathered rows"
            lw = p.log_w[:n0].cpu()
            if d.resampled:
                assert bool((lw == lw[0]).all()) and abs(float(lw[0]) - d.log_w_common) <= 1e-6 * max(1.0, abs(d.log_w_common))
            else:
                assert torch.equal(lw, lw_before[:n0].cpu())
            p.plain(0, j, j)                             # transition j from the resampled point
            assert torch.isfinite(p.log_w[:n0]).all() and torch.isfinite(p.x[:n0]).all()
        assert fired == M if tau > 1 else 0 < fired      # (at TAU_MID too some step compares stratified ancestors)


@pytest.mark.parametrize("hmc", [True, False])
def test_systematic_through_the_new_argument_is_bit_identical(hmc):
    """resample_method="systematic" (method 0 passed explicitly) against the call that does not pass the argument at all."""
    B = 100
    eps0, na, nb, nr = base.inputs(B, seed=3, hmc=hmc, kill=(1,))
    dev = lambda *ts: tuple(t.to(DEV) for t in ts)      # noqa: E731
    runs = []
    for explicit in (False, True):
        _, hf, target, op, ais = base.samplers(hmc=hmc, tau=TAU_MID, eval_mode=False)
        if explicit:
            ais.resample_method = "systematic"
            pt, log_w, n_valid, stats, _, _ = ais.run(B, *dev(eps0, na, nb), noise_r=nr.to(DEV), trace=True)
            out = (pt.x, pt.log_q, pt.log_p, log_w, n_valid, stats[:6], *ais.last_smc)
        else:                                            # the op as the parent commit's package called it: no trailing argument
            ops = _ops.load()
            slots = ((op.epsilons, op.common_epsilon, op.mass_vector, 1, base.L, float(op.max_grad), float(op.target_p_accept), True)
                     if hmc else (op.noise_scalings, None, None, 2, 0, 0.0, float(op.target_prob_accept), True))
            o = ops.ais_run_ext(*hf.native(), *target.native_target(), ais._betas(), 2.0, False,
                                _ops.TRANSITION_HMC if hmc else _ops.TRANSITION_METROPOLIS, *dev(eps0, na, nb), *slots,
                                None, None, None, None, False, 0, TAU_MID, nr.to(DEV), True)
            out = (o[0], o[1], o[2], o[5], o[6], o[7][:6], *o[10:14])
        runs.append(out)
    n1 = int(runs[0][4][1])
    assert n1 == B - 1 and 0 < int(runs[0][6].sum())
    cut = lambda t: t[:n1] if t.dim() >= 1 and t.shape[0] == B else t      # noqa: E731
    for i, (u, v) in enumerate(zip(*runs)):
        assert torch.equal(cut(u), cut(v)), f"output {i} differs"
    # the decision op alone: method 0 explicit, method 0 by default, and method 1 differs in the ancestors only
    lw = (torch.randn(257, generator=torch.Generator().manual_seed(9)) * 1.5).to(DEV)      # (far from degenerate)
    u = nr[:1].to(DEV)
    ops = _ops.load()
    a, b, c = ops.smc_decide(lw, 1.5, u), ops.smc_decide(lw, 1.5, u, 0), ops.smc_decide(lw, 1.5, u, STRATIFIED)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], c[0]) and all(torch.equal(x, y) for x, y in zip(a[1:], c[1:]))
    np.testing.assert_array_equal(a[0].cpu().numpy(), smc_spec.decide(lw.cpu().numpy(), 1.5, float(u)).ancestors)
    np.testing.assert_array_equal(c[0].cpu().numpy(), sspec.decide(lw.cpu().numpy(), 1.5, float(u)).ancestors)
    with pytest.raises(Exception):
        ops.smc_decide(lw, 1.5, u, 2)


@pytest.mark.parametrize("hmc", [True, False])
def test_fused_call_equals_the_phased_call_and_is_deterministic(hmc):
    B = 100
    eps0, na, nb, nr = base.inputs(B, seed=3, hmc=hmc, kill=(1,))
    runs = []
    for _ in range(2):
        _, _, _, op, ais = samplers(hmc=hmc, tau=TAU_MID, eval_mode=False)
        pt, log_w, n_valid, stats, _, _ = ais.run(B, eps0.to(DEV), na.to(DEV), nb.to(DEV), noise_r=nr.to(DEV), trace=True)
        st = (op.epsilons.clone(), op.common_epsilon.clone()) if hmc else (op.noise_scalings.clone(),)
        runs.append((pt.x, pt.log_q, pt.log_p, log_w, n_valid, stats[:6], *ais.last_smc, *st))
    n1 = int(runs[0][4][1])
    assert n1 == B - 1
    cut = lambda t: t[:n1] if t.dim() >= 1 and t.shape[0] == B else t      # noqa: E731
    for i, (u, v) in enumerate(zip(*runs)):
        assert torch.equal(cut(u), cut(v)), f"two identical calls differ in output {i}"
    _, _, _, op, ais = samplers(hmc=hmc, tau=TAU_MID, eval_mode=False)
    p = Phased(ais, B, eps0, na, nb, nr)
    p.smc(1, 1, 0, TAU_MID)
    for j in range(1, M + 1):
        p.smc(0, j, j, TAU_MID)
    p.smc(2, 1, 0, TAU_MID)
    st = (op.epsilons, op.common_epsilon) if hmc else (op.noise_scalings,)
    phased = (p.x, p.lq, p.lp, p.log_w, p.n_valid, p.stats[:6], p.resampled, p.ess, p.ancestors, p.log_w_pre, *st)
    for i, (u, v) in enumerate(zip(runs[0], phased)):
        assert torch.equal(cut(u), cut(v)), f"fused and phased calls differ in output {i}"
    n0 = int(p.n_valid[0])
    for j in range(M):
        check_decision(p.log_w_pre[j], n0, TAU_MID, nr[j], p.ancestors[j], p.resampled[j], p.ess[j], f"transition {j + 1}")


def test_generic_path_follows_the_spec():
    from torch_dist_plugin import WrappedTorchDist
    Dg, Mg, B = 6, 4, 100
    torch.manual_seed(0)
    dist = WrappedTorchDist(torch.distributions.MultivariateNormal(torch.zeros(Dg, device=DEV),
                                                                   scale_tril=1.5 * torch.eye(Dg, device=DEV)))
    target = fa.ManyWellEnergy(Dg)
    for tau in (1.5, 0.2):
        hmc = fa.HamiltonianMonteCarlo(Mg, Dg, dist.log_prob, target.log_prob, alpha=2.0, p_target=True, epsilon=0.2, L=3).to(DEV)
        ais = fa.AnnealedImportanceSampler(dist, target.log_prob, hmc, True, None, Mg, resample_threshold=tau,
                                           resample_method="stratified")
        assert not ais.is_native
        nr = torch.rand(Mg, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        pt, lw = ais.sample_and_log_weights(B, noise_r=nr.to(DEV))
        resampled, ess, anc, lw_pre = ais.last_smc
        assert pt.x.shape == (B, Dg) and torch.isfinite(lw).all()
        for j in range(Mg):
            check_decision(lw_pre[j], B, tau, nr[j], anc[j], resampled[j], ess[j], f"generic, tau {tau}, transition {j + 1}")
        assert int(resampled.sum()) == Mg or tau < 1


def test_defensive_mixture_call_follows_the_spec():
    B = 100
    eps0, na, nb, nr = base.inputs(B, seed=6)
    nf = base.seeded_oracle_flow(D, base.K, base.NODES, 7, std=0.01)
    mix = fa.DefensiveMixtureDistribution(base.hip_flow(nf)).to(DEV).requires_grad_(False)
    target = fa.ManyWellEnergy(D)
    op = fa.HamiltonianMonteCarlo(M, D, mix.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=base.STEP, L=base.L,
                                  eval_mode=True).to(DEV)
    sel = torch.rand(B, generator=torch.Generator().manual_seed(8))
    for tau in (1.5, TAU_MID):
        ais = fa.AnnealedImportanceSampler(mix, target.log_prob, op, False, 2.0, M, resample_threshold=tau,
                                           resample_method="stratified")
        pt, log_w, n_valid, stats, _, _ = ais.run(B, eps0.to(DEV), na.to(DEV), nb.to(DEV), noise_r=nr.to(DEV), trace=True,
                                                  sel=sel.to(DEV))
        resampled, ess, anc, lw_pre = ais.last_smc
        n0 = int(n_valid[0])
        assert n0 == B and anc.shape == (M, B)
        for j in range(M):
            check_decision(lw_pre[j], n0, tau, nr[j], anc[j], resampled[j], ess[j], f"mixture, tau {tau}, transition {j + 1}")
        assert int(resampled.sum()) == M or tau < 1


def test_call_with_stratified_resampling_replays_from_a_hip_graph():
    """One captured call (a single stream, no parallel branches) replays on two sets of inputs and gives what the eager call
    gives on each."""
    B = 256
    _, _, _, op, ais = samplers(tau=1.5)
    e0, a0, b0, r0 = (t.to(DEV) for t in base.inputs(B, seed=4))
    e1, a1, b1, r1 = (t.to(DEV) for t in base.inputs(B, seed=5))
    s_eps, s_a, s_b, s_r = e0.clone(), a0.clone(), b0.clone(), r0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ais.run(B, s_eps, s_a, s_b, noise_r=s_r, trace=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pt, log_w, n_valid, stats, _, _ = ais.run(B, s_eps, s_a, s_b, noise_r=s_r, trace=True)
        resampled, ess, anc, lw_pre = ais.last_smc
    for e, a, b, r in ((e0, a0, b0, r0), (e1, a1, b1, r1)):
        s_eps.copy_(e); s_a.copy_(a); s_b.copy_(b); s_r.copy_(r)
        g.replay(); torch.cuda.synchronize()
        got = (pt.x.clone(), log_w.clone(), resampled.clone(), anc.clone())
        pe, lwe, _, _, _, _ = ais.run(B, e, a, b, noise_r=r, trace=True)
        want = (pe.x, lwe, ais.last_smc[0], ais.last_smc[2])
        assert all(torch.equal(u, v) for u, v in zip(got, want))
        assert int(resampled.sum()) == M
        check_decision(lw_pre[0], B, 1.5, r[0], anc[0], resampled[0], ess[0], "replayed transition 1")


def test_python_surface_and_refusals():
    B = 64
    _, _, _, op, ais = base.samplers(tau=None)
    assert ais.resample_method == "systematic"
    ais.resample_method = "stratified"                   # allowed and inert without a threshold
    torch.manual_seed(0)
    pt, lw = ais.sample_and_log_weights(B)
    assert torch.isfinite(lw).all() and "n_resampled" not in ais.get_logging_info()
    with pytest.raises(_ops.FabhipError, match="resample_method"):
        ais.resample_method = "multinomial"
    with pytest.raises(_ops.FabhipError, match="resample_method"):
        fa.AnnealedImportanceSampler(ais.base_distribution, ais.target_log_prob, op, False, 2.0, M, resample_method=1)
    ais.resample_threshold = 1.5
    ais.sample_and_log_weights(B)
    assert ais.get_logging_info()["n_resampled"] == M
    # FABModel hands the setting to its sampler
    model = fa.FABModel(ais.base_distribution, fa.ManyWellEnergy(D), M, alpha=2.0, transition_operator=op, loss_type="fab_alpha_div",
                        ais_resample_threshold=0.5, ais_resample_method="stratified")
    assert model.annealed_importance_sampler.resample_method == "stratified"
    assert model.annealed_importance_sampler.resample_threshold == 0.5
    with pytest.raises(_ops.FabhipError, match="resample_method"):
        fa.FABModel(ais.base_distribution, fa.ManyWellEnergy(D), M, alpha=2.0, transition_operator=op, loss_type="fab_alpha_div",
                    ais_resample_method="residual")
    # the resampling step over ranks is systematic: a stratified sampler is refused by name
    sh = parallel.ShardedAnnealedImportanceSampler(ais, resample_across_ranks=True)
    with pytest.raises(_ops.FabhipError, match="resample_method"):
        sh.sample_and_log_weights(B)
    ais.resample_method = "systematic"
    x, lw, lq = sh.sample_and_log_weights(B)
    assert x.shape == (B, D) and torch.isfinite(lw).all()
