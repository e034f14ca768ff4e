"""SMC mode of the fused AIS call on the GPU (resample_threshold; include/fabhip.h: fabhip_smc_args) against its specification
(tests/smc_spec.py).  A free-running comparison of a whole call is the wrong test here - one flipped accept decision shifts the
CDF and with it the ancestors of many chains - so every decision is teacher-forced: the device's own `log_w_pre[j]` goes into the
spec, whose ancestors and decision must be EQUAL to the device's, its ess and common log-weight within float32 rounding.

Inputs are benign in the sense of tests/test_gpu_parity.py (headline-architecture test in the mild regime): the last coupling
Linears are N(0, 0.01^2) and the step size is 0.05, so one transition does not amplify fp32 rounding and every accept margin is
far from its threshold - no float64 arbitration is needed and a flipped accept decision is a failure.  (The rule the other parity
tests apply to fragile chains - a differing decision must sit inside the rounding band of its threshold, re-evaluated in float64,
at most B / 8 chains per transition - is therefore not used; the test asserts that no decision differs.)"""
import numpy as np
import pytest
import torch

from helpers import close, max_rel_err, seeded_oracle_flow, RTOL
import smc_spec

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops            # noqa: E402
from oracle import ais as oais            # noqa: E402
from oracle import targets as otgt        # noqa: E402

DEV = "cuda"
D, K, NODES, M, L, STEP = 32, 3, 10, 4, 3, 0.05
TAU_MID = 0.05       # see test_thresholds_are_not_coin_flips: every ess of these runs is > 1e-3 (relative) away from it


def hip_flow(nf):
    f = fa.RealNVP(D, K, NODES)
    f._nf_model.load_state_dict(nf.state_dict())
    return f.to(DEV).requires_grad_(False)


def inputs(B, seed=0, hmc=True, kill=()):
    g = torch.Generator().manual_seed(100 + seed)
    eps0 = torch.randn(B, D, generator=g)
    for r in kill:                                        # a chain the "chain init" filter removes (x = inf)
        eps0[r] = float("inf")
    n_inner = 1 if hmc else 2
    na = torch.randn(M, n_inner, B, D, generator=g)
    nb = torch.empty(M, n_inner, B).exponential_(1.0, generator=g) if hmc else torch.rand(M, n_inner, B, generator=g)
    nr = torch.rand(M, generator=g, dtype=torch.float64)
    return eps0, na, nb, nr


def samplers(hmc=True, tau=None, eval_mode=True, nf=None):
    nf = seeded_oracle_flow(D, K, NODES, 7, std=0.01) if nf is None else nf
    hf = hip_flow(nf)
    target = fa.ManyWellEnergy(D)
    if hmc:
        op = fa.HamiltonianMonteCarlo(M, D, hf.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=STEP, L=L,
                                      eval_mode=eval_mode).to(DEV)
    else:
        op = fa.Metropolis(M, D, hf.log_prob, target.log_prob, n_updates=2, alpha=2.0, p_target=False, max_step_size=0.05,
                           min_step_size=0.02, eval_mode=eval_mode).to(DEV)
    ais = fa.AnnealedImportanceSampler(hf, target.log_prob, op, False, 2.0, M, resample_threshold=tau)
    return nf, hf, target, op, ais


def oracle_op(nf, hmc=True):
    ot = otgt.ManyWell(D)
    if hmc:
        return oais.HMC(M, D, nf.log_prob, ot.log_prob, alpha=2.0, p_target=False, epsilon=STEP, L=L, eval_mode=True)
    return oais.Metropolis(M, D, nf.log_prob, ot.log_prob, n_updates=2, alpha=2.0, p_target=False, max_step_size=0.05,
                           min_step_size=0.02, eval_mode=True)


class Phased:
    """One AIS run stepped through torch.ops.fabhip.ais_phase_smc / ais_phase on caller-owned state."""

    def __init__(self, ais, B, eps0, na, nb, nr):
        self.ais, self.B = ais, B
        self.flow, self.target = ais._native_parts()
        self.op = ais.transition_operator
        self.hmc = isinstance(self.op, fa.HamiltonianMonteCarlo)
        f32 = dict(dtype=torch.float32, device=DEV)
        self.x, self.lq, self.lp = torch.empty(B, D, **f32), torch.empty(B, **f32), torch.empty(B, **f32)
        self.gq = torch.empty(B, D, **f32) if self.hmc else None
        self.gp = torch.empty(B, D, **f32) if self.hmc else None
        self.log_w = torch.empty(B, **f32)
        self.n_valid = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.stats = torch.zeros(16, **f32)
        self.eps0, self.na, self.nb, self.nr = eps0.to(DEV), na.to(DEV).contiguous(), nb.to(DEV).contiguous(), nr.to(DEV)
        self.resampled = torch.full((M,), -1, dtype=torch.int32, device=DEV)
        self.ess = torch.full((M,), -1.0, **f32)
        self.ancestors = torch.full((M, B), -1, dtype=torch.int32, device=DEV)
        self.log_w_pre = torch.full((M, B), float("nan"), **f32)

    def _common(self, phases, j0, j1):
        op, a = self.op, self.ais
        head = (*self.flow.native(), *self.target.native_target(), a._betas(), 2.0, False,
                _ops.TRANSITION_HMC if self.hmc else _ops.TRANSITION_METROPOLIS, int(phases), int(j0), int(j1), self.eps0, self.na,
                self.nb)
        if self.hmc:
            mid = (op.epsilons, op.common_epsilon, op.mass_vector, op.n_outer, op.L, float(op.max_grad), float(op.target_p_accept),
                   not op.eval_mode)
        else:
            mid = (op.noise_scalings, None, None, op.n_updates, 0, 0.0, float(op.target_prob_accept),
                   bool(op.adjust_step_size and not op.eval_mode))
        tail = (self.x, self.lq, self.lp, self.gq, self.gp, self.log_w, self.n_valid, self.stats, None, None, None, None, None,
                None, None, _ops.precision_of(self.flow))
        return head + mid + tail

    def plain(self, phases, j0, j1):
        _ops.load().ais_phase(*self._common(phases, j0, j1))

    def smc(self, phases, j0, j1, tau, only_resample=False):
        _ops.load().ais_phase_smc(*self._common(phases, j0, j1), tau, self.nr if tau is not None else None, bool(only_resample),
                                  self.resampled, self.ess, self.ancestors, self.log_w_pre)

    def point(self):
        c = lambda t: None if t is None else t.clone()      # noqa: E731
        return c(self.x), c(self.lq), c(self.lp), c(self.gq), c(self.gp)


def check_decision(log_w_pre, n0, tau, u, anc_dev, resampled_dev, ess_dev, tag):
    """The device's decision against the spec fed with the weights the device saw."""
    d = smc_spec.decide(log_w_pre[:n0].cpu().numpy(), tau, float(u))
    assert abs(d.ess - tau) >= 1e-3 * tau, f"{tag}: ess {d.ess} within 1e-3 of tau {tau}: the decision is a coin flip"
    assert bool(resampled_dev) == d.resampled, f"{tag}: decision differs (spec ess {d.ess}, device ess {float(ess_dev)})"
    assert abs(float(ess_dev) - d.ess) <= 1e-6 * d.ess, f"{tag}: ess {float(ess_dev)} vs {d.ess}"
    anc = anc_dev.cpu().numpy().astype(np.int64)
    assert np.array_equal(anc[:n0], d.ancestors), f"{tag}: {int((anc[:n0] != d.ancestors).sum())} ancestors differ"
    assert np.array_equal(anc[n0:], np.arange(n0, anc.shape[0])), f"{tag}: rows beyond n0 must map to themselves"
    return d


# ---- 5. the new entry points with the mode off -----------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_threshold_none_through_the_new_ops_is_bit_identical(hmc):
    B = 200
    eps0, na, nb, nr = inputs(B, hmc=hmc, kill=(5,))
    outs = []
    for smc in (False, True):
        _, hf, target, op, ais = samplers(hmc=hmc, eval_mode=False)
        ops = _ops.load()
        call = ops.ais_run_ext if smc else ops.ais_run
        extra = (None, None, False) if smc else ()
        if hmc:
            o = call(*hf.native(), *target.native_target(), ais._betas(), 2.0, False, _ops.TRANSITION_HMC, eps0.to(DEV), na.to(DEV),
                     nb.to(DEV), op.epsilons, op.common_epsilon, op.mass_vector, 1, L, float(op.max_grad), float(op.target_p_accept),
                     True, None, None, None, None, False, 0, *extra)
        else:
            o = call(*hf.native(), *target.native_target(), ais._betas(), 2.0, False, _ops.TRANSITION_METROPOLIS, eps0.to(DEV),
                     na.to(DEV), nb.to(DEV), op.noise_scalings, None, None, 2, 0, 0.0, float(op.target_prob_accept), True, None, None,
                     None, None, False, 0, *extra)
        state = (op.epsilons.clone(), op.common_epsilon.clone()) if hmc else (op.noise_scalings.clone(),)
        outs.append((list(o[:10]), state, list(o[10:])))
    (a, sa, _), (b, sb, extra) = outs
    n1 = int(a[6][1])
    assert int(a[6][0]) == B - 1 and torch.equal(a[6], b[6])
    for i, (u, v) in enumerate(zip(a, b)):
        u, v = (u[:n1], v[:n1]) if i < 6 and u.numel() else (u, v)
        assert torch.equal(u, v), f"output {i} differs"
    assert all(torch.equal(u, v) for u, v in zip(sa, sb))
    assert all(t.numel() == 0 for t in extra)
    # the phased op with the mode off against the plain phased op
    res = []
    for smc in (False, True):
        _, _, _, _, ais = samplers(hmc=hmc, eval_mode=False)
        p = Phased(ais, B, eps0, na, nb, nr)
        (p.smc(3, 1, M, None) if smc else p.plain(3, 1, M))
        res.append((p.x, p.lq, p.lp, p.log_w, p.n_valid, p.stats[:6]))
    n1 = int(res[0][4][1])
    assert all(torch.equal(u[:n1] if u.shape[0] == B else u, v[:n1] if v.shape[0] == B else v) for u, v in zip(*res))


# ---- 6. the decisions, teacher-forced ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
@pytest.mark.parametrize("tau", [1.5, TAU_MID])
def test_decisions_and_ancestors_equal_the_spec(tau, hmc):
    B = 300
    eps0, na, nb, nr = inputs(B, seed=1, hmc=hmc)
    _, _, _, _, ais = samplers(hmc=hmc, tau=tau)
    pt, log_w, n_valid, stats, _, _ = ais.run(B, eps0.to(DEV), na.to(DEV), nb.to(DEV), noise_r=nr.to(DEV), trace=True)
    resampled, ess, anc, lw_pre = ais.last_smc
    n0 = int(n_valid[0])
    assert n0 == B and resampled.shape == (M,) and anc.shape == (M, B) and lw_pre.shape == (M, B)
    fired = 0
    for j in range(M):
        d = check_decision(lw_pre[j], n0, tau, nr[j], anc[j], resampled[j], ess[j], f"transition {j + 1}")
        fired += d.resampled
    assert fired == M if tau > 1 else 0 < fired
    assert torch.isfinite(log_w).all() and int(n_valid[1]) == B


def test_thresholds_are_not_coin_flips():
    """The CPU spec alone on the inputs of the tests that run with TAU_MID: every ess is at least a relative 1e-2 away from it (the
    device-side tests assert 1e-3 on the device's own weights), and both outcomes of the decision occur."""
    for hmc in (True, False):
        for B, seed, kill in ((300, 1, ()), (100, 3, (1,)), (1500, 3, (1,)), (256, 4, ()), (256, 5, ())):
            eps0, na, nb, nr = inputs(B, seed=seed, hmc=hmc, kill=kill)
            nf = seeded_oracle_flow(D, K, NODES, 7, std=0.01)
            ot = otgt.ManyWell(D)
            s = smc_spec.SMC(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, ot.log_prob, oracle_op(nf, hmc),
                             False, 2.0, M, resample_threshold=TAU_MID)
            s.sample_and_log_weights(eps0, na, nb, noise_r=nr)
            print(hmc, B, [round(e, 4) for e in s.trace.ess], s.trace.resampled)
            assert all(abs(e - TAU_MID) >= 1e-2 * TAU_MID for e in s.trace.ess)
            assert any(s.trace.resampled) and not all(s.trace.resampled)


# ---- 7. the gather and the transition that follows, phase by phase -----------------------------------------------------------------
@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("shape,B,kill", [(16, 100, ()), (8, 100, ()), (4, 101, ()), (4, 100, (3, 40)), (8, 99, (0,)), (16, 64, (63,))])
def test_gather_is_bit_exact_and_the_next_transition_matches_the_oracle(shape, B, kill, fast):
    eps0, na, nb, nr = inputs(B, seed=2, kill=kill)
    nf, hf, target, op, ais = samplers(tau=1.5)
    ohmc = oracle_op(nf)
    with _ops.option(_ops.OPT_TILE_SHAPE, shape), fa.fast_mode(fast):
        p = Phased(ais, B, eps0, na, nb, nr)
        p.smc(1, 1, 0, 1.5)                              # FABHIP_AIS_INIT
        n0 = int(p.n_valid[0])
        assert n0 == B - len(kill)
        for j in range(1, M + 1):
            before, lw_before = p.point(), p.log_w.clone()
            p.smc(0, j, j, 1.5, only_resample=True)
            assert torch.equal(p.log_w_pre[j - 1][:n0], lw_before[:n0])
            d = check_decision(p.log_w_pre[j - 1], n0, 1.5, nr[j - 1], p.ancestors[j - 1], p.resampled[j - 1], p.ess[j - 1],
                               f"transition {j}")
            idx = p.ancestors[j - 1].long()
            after = p.point()
            for name, u, v in zip(("x", "log_q", "log_p", "grad_log_q", "grad_log_p"), before, after):
                assert torch.equal(v[:n0], u[idx[:n0]]), f"transition {j}: {name} is not the gathered rows"
                assert torch.equal(v[n0:].isnan(), u[n0:].isnan()) and torch.equal(v[n0:].nan_to_num(), u[n0:].nan_to_num())
            lw = p.log_w[:n0].cpu()
            assert bool((lw == lw[0]).all()) and abs(float(lw[0]) - d.log_w_common) <= 1e-6 * max(1.0, abs(d.log_w_common))
            # transition j from the resampled point: the plain phase op against the oracle's transition
            start = oais.Point(*[t[:n0].cpu().clone() for t in after])
            p.plain(0, j, j)
            if fast:       # bf16 conditioner GEMMs: no fp32-oracle parity by design (tests/test_gpu_fast_mode.py compares them with
                assert torch.isfinite(p.log_w[:n0]).all() and torch.isfinite(p.x[:n0]).all()      # their own emulation): the
                continue                                                                          # resampling half is the subject
            out = ohmc.transition(start, j, ais.B_space[j], na[j - 1], nb[j - 1])
            moved = (p.x[:n0].cpu() != after[0][:n0].cpu()).any(1)
            assert torch.equal(moved, ohmc.last_accept), f"transition {j}: an accept decision differs from the oracle"
            assert max_rel_err(p.x[:n0], out.x) <= RTOL, f"transition {j}: x err {max_rel_err(p.x[:n0], out.x):.2e}"
            assert close(p.lq[:n0], out.log_q, RTOL) and close(p.lp[:n0], out.log_p, RTOL), f"transition {j}: densities"
            b, bn = ais.B_space[j], ais.B_space[j + 1]
            inc = oais.intermediate_log_prob(out, bn, 2.0, False) - oais.intermediate_log_prob(out, b, 2.0, False)
            assert close(p.log_w[:n0], torch.full((n0,), d.log_w_common) + inc.float(), RTOL, atol_scale=4)


# ---- 8. fused == phased, determinism, graph capture -----------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
@pytest.mark.parametrize("B", [100, 1500])
def test_fused_call_equals_the_phased_call_and_is_deterministic(B, hmc):
    eps0, na, nb, nr = inputs(B, seed=3, hmc=hmc, kill=(1,))
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
    assert 0 < int(p.resampled.sum()) <= M


def test_call_with_resampling_replays_from_a_hip_graph():
    """The launch sequence does not depend on the device flag: one captured call (a single stream, no parallel branches) replays
    on two sets of inputs - their decisions differ - and gives what the eager call gives on each."""
    B = 256
    _, _, _, op, ais = samplers(tau=TAU_MID)
    e0, a0, b0, r0 = (t.to(DEV) for t in inputs(B, seed=4))
    e1, a1, b1, r1 = (t.to(DEV) for t in inputs(B, seed=5))
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
        assert 0 < int(resampled.sum())


# ---- 9. generic plug-in path -------------------------------------------------------------------------------------------------------
def test_generic_path_follows_the_spec():
    from torch_dist_plugin import WrappedTorchDist
    Dg, Mg, B = 6, 4, 256
    torch.manual_seed(0)
    base = WrappedTorchDist(torch.distributions.MultivariateNormal(torch.zeros(Dg, device=DEV),
                                                                   scale_tril=1.5 * torch.eye(Dg, device=DEV)))
    target = fa.ManyWellEnergy(Dg)
    for tau in (1.5, 0.2):
        hmc = fa.HamiltonianMonteCarlo(Mg, Dg, base.log_prob, target.log_prob, alpha=2.0, p_target=True, epsilon=0.2, L=3).to(DEV)
        ais = fa.AnnealedImportanceSampler(base, target.log_prob, hmc, True, None, Mg, resample_threshold=tau)
        assert not ais.is_native
        nr = torch.rand(Mg, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        pt, lw = ais.sample_and_log_weights(B, noise_r=nr.to(DEV))
        resampled, ess, anc, lw_pre = ais.last_smc
        assert pt.x.shape == (B, Dg) and torch.isfinite(lw).all()
        for j in range(Mg):
            check_decision(lw_pre[j], B, tau, nr[j], anc[j], resampled[j], ess[j], f"generic, tau {tau}, transition {j + 1}")
        info = ais.get_logging_info()
        assert info["n_resampled"] == int(resampled.sum()) and abs(info["ess_min_in_chain"] - float(ess.min())) < 1e-6
        assert info["n_resampled"] == Mg or tau < 1
        assert abs(info["log_Z"] - float(target.log_Z)) < 1.5


# ---- 10. trainer smoke + the Python surface ----------------------------------------------------------------------------------------
def test_trainer_runs_with_resampling_on():
    Dt, Mt, B = 6, 4, 256
    torch.manual_seed(1)
    flow = fa.make_wrapped_normflow_realnvp(Dt, 4, 10, act_norm=False).to(DEV)
    target = fa.ManyWellEnergy(Dt)
    hmc = fa.HamiltonianMonteCarlo(Mt, Dt, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.2, L=5).to(DEV)
    model = fa.FABModel(flow, target, Mt, alpha=2.0, transition_operator=hmc, loss_type="fab_alpha_div",
                        ais_resample_threshold=0.5)
    ais = model.annealed_importance_sampler
    assert ais.resample_threshold == 0.5

    def initial_sampler():
        pt, lw = ais.sample_and_log_weights(B, logging=False)
        return pt.x, lw, pt.log_q
    buf = fa.PrioritisedReplayBuffer(Dt, 8 * B, 2 * B, initial_sampler, device=DEV)
    opt = fa.FlatAdam(flow, lr=1e-4)
    trainer = fa.PrioritisedBufferTrainer(model, opt, buf, alpha=2.0, n_batches_buffer_sampling=2)
    for i in range(4):
        info = trainer.step(i, B)
        assert np.isfinite(info["loss"]), (i, info)
        assert 0 <= info["n_resampled"] <= Mt and 0 < info["ess_min_in_chain"] <= 1.0 + 1e-6
        assert 0 < info["ess_ais"] <= 1 and np.isfinite(info["log_Z"])
    assert buf.current_index == 2 * B + 4 * B and not buf.is_full                  # two initial calls + one per iteration
    assert torch.isfinite(buf.buffer.log_w[:buf.current_index]).all() and torch.isfinite(buf.buffer.x[:buf.current_index]).all()


def test_logging_keys_prefetch_bypass_and_refusals():
    B = 128
    _, _, _, op, ais = samplers(tau=None)
    torch.manual_seed(0)
    for _ in range(3):
        ais.sample_and_log_weights(B)
    assert "_pf_state" in ais.__dict__ and "n_resampled" not in ais.get_logging_info()
    ais.resample_threshold = 1.5                         # settable; the prefetched piece is dropped, the mode's calls are one-op calls
    for _ in range(2):
        pt, lw = ais.sample_and_log_weights(B)
    info = ais.get_logging_info()
    assert "_pf_state" not in ais.__dict__ and info["n_resampled"] == M and 0 < info["ess_min_in_chain"] <= 1
    assert torch.isfinite(lw).all() and pt.x.shape == (B, D)
    ais.resample_threshold = 0.0
    ais.sample_and_log_weights(B)
    assert ais.get_logging_info()["n_resampled"] == 0
    with pytest.raises(_ops.FabhipError, match="noise_r"):
        ais.sample_and_log_weights(B, noise_r=torch.rand(M, device=DEV))                  # float32
    with pytest.raises(_ops.FabhipError, match="noise_r"):
        ais.sample_and_log_weights(B, noise_r=torch.rand(M + 1, dtype=torch.float64, device=DEV))
    ais.resample_threshold = None
    with pytest.raises(_ops.FabhipError, match="resample_threshold"):
        ais.sample_and_log_weights(B, noise_r=torch.rand(M, dtype=torch.float64, device=DEV))
    # sharded chains with the setting: refused by name
    ais.resample_threshold = 0.5
    from fab_torch_amd import parallel
    sh = parallel.ShardedAnnealedImportanceSampler(ais)
    with pytest.raises(_ops.FabhipError, match="resample_threshold"):
        sh.sample_and_log_weights(B)
    with pytest.raises(_ops.FabhipError, match="resample_threshold"):
        parallel.ShardedAIS(ais.sample_and_log_weights).sample_and_log_weights(B)
