"""CPU tests of the adaptive schedule's specification (tests/adaptive_spec.py) and of the host side of the product's settings: custom
schedules, `ess_decay`, and the routes that refuse distribution_spacing_type="adaptive".  No GPU."""
import math

import numpy as np
import pytest
import torch

from helpers import seeded_oracle_flow
from oracle import ais as oais, targets as otgt
import adaptive_spec
import smc_spec
from adaptive_spec import next_beta


def _setup(D=6, B=64, M=3, seed=0, hmc=True, eps=0.2, p_target=False):
    """tests/test_smc_spec.py's setup."""
    nf = seeded_oracle_flow(D, 4, 10, 3)
    tg = otgt.ManyWell(D)
    if hmc:
        op = oais.HMC(M, D, nf.log_prob, tg.log_prob, alpha=2.0, p_target=p_target, epsilon=eps, L=5, eval_mode=True)
    else:
        op = oais.Metropolis(M, D, nf.log_prob, tg.log_prob, n_updates=2, alpha=2.0, p_target=p_target, eval_mode=True)
    g = torch.Generator().manual_seed(seed)
    eps0 = torch.randn(B, D, generator=g)
    n_inner = 1 if hmc else 2
    na = torch.randn(M, n_inner, B, D, generator=g)
    nb = torch.empty(M, n_inner, B).exponential_(1.0, generator=g) if hmc else torch.rand(M, n_inner, B, generator=g)
    nr = torch.rand(M, generator=g, dtype=torch.float64)
    sample = lambda e: tuple(t.detach() for t in nf.sample_eps(e))      # noqa: E731
    mk = lambda cls, **kw: cls(sample, nf.log_prob, tg.log_prob, op, p_target, 2.0, M, **kw)      # noqa: E731
    return mk, (eps0, na, nb, nr), tg


def _weights(n, scale, seed=0):
    g = np.random.default_rng(seed)
    lw = g.normal(size=n).astype(np.float32)
    lq = g.normal(size=n).astype(np.float32)
    lp = (lq + np.float32(scale) * g.normal(size=n).astype(np.float32)).astype(np.float32)
    return lw, lq, lp


# ---- next_beta ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.01, 5.0, 1e9])
def test_one_live_row_always_answers_one(scale):
    """ESS >= 1 / n0 whatever the weights: with n0 = 1 every candidate has ESS 1 >= rho."""
    lw, lq, lp = _weights(1, scale)
    for rho in (0.5, 0.9, 0.999):
        r = next_beta(lw, lq, lp, 0.0, 2.0, False, rho)
        assert r == adaptive_spec.NextBeta(1.0, 1.0, 1.0, 2, False)


@pytest.mark.parametrize("scale", [0.01, 5.0, 1e9])
def test_two_rows_at_half_answer_one(scale):
    """n0 = 2: ESS >= 1 / 2 >= 0.5 ess0 for every ess0 <= 1."""
    lw, lq, lp = _weights(2, scale, seed=1)
    assert next_beta(lw, lq, lp, 0.25, 2.0, False, 0.5).beta_next == 1.0


def test_beta_one_answers_one_with_one_evaluation():
    lw, lq, lp = _weights(100, 5.0)
    r = next_beta(lw, lq, lp, 1.0, 2.0, False, 0.7)
    assert r.beta_next == 1.0 and r.evaluations == 1 and not r.floor and r.ess_choice == r.ess0 > 0


def test_no_finite_weight_answers_one():
    lw, lq, lp = _weights(50, 5.0)
    r = next_beta(np.full(50, np.nan, np.float32), lq, lp, 0.3, 2.0, False, 0.7)
    assert r == adaptive_spec.NextBeta(1.0, 0.0, 0.0, 2, False)


def test_tiny_spread_answers_one_with_two_evaluations():
    lw, lq, lp = _weights(500, 1e-4)
    r = next_beta(lw, lq, lp, 0.0, 2.0, False, 0.7)
    assert r.beta_next == 1.0 and r.evaluations == 2 and not r.floor and r.ess_choice >= 0.7 * r.ess0


@pytest.mark.parametrize("beta", [0.0, 0.25])
def test_huge_spread_takes_the_floor(beta):
    lw, lq, lp = _weights(500, 1e9)
    r = next_beta(lw, lq, lp, beta, 2.0, False, 0.7)
    assert r.floor and r.evaluations == 26 and r.beta_next == beta + (1.0 - beta) / 2 ** 24
    assert r.ess_choice < 0.7 * r.ess0


@pytest.mark.parametrize("p_target", [False, True])
@pytest.mark.parametrize("rho", [0.5, 0.9])
@pytest.mark.parametrize("beta", [0.0, 0.25, 1 - 2.0 ** -20])
def test_interior_choice_keeps_the_threshold(beta, rho, p_target):
    n = 700
    lw, lq, lp = _weights(n, 5.0 / (1.0 - beta), seed=2)        # (the spread of room * d is ~5 at every beta)
    lw[3], lw[10], lw[11], lp[20] = np.nan, np.inf, -np.inf, -np.inf
    r = next_beta(lw, lq, lp, beta, 2.0, p_target, rho)
    assert beta < r.beta_next < 1.0 and not r.floor and r.evaluations == 26
    assert r.ess_choice >= rho * r.ess0 and 1.0 / n <= r.ess0 <= 1.0


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
@pytest.mark.parametrize("tau", [None, 0.5])
def test_forced_linear_schedule_is_the_oracle(hmc, tau):
    """The driver on the linear B_space against oracle.ais.AIS / smc_spec.SMC.  The beta_1 := 0 start splits the first weight into
    two adds (pi_0 - log q0, then pi_beta1 - pi_0), so log_w agrees to float32 rounding, 1e-6 as in tests/test_gpu_smc.py, not bit for
    bit; the points are the oracle's own (no weight enters a transition; with tau the decisions see weights that differ by that
    rounding, and must still agree)."""
    mk, (eps0, na, nb, nr), _ = _setup(hmc=hmc)
    ref = mk(smc_spec.SMC, resample_threshold=tau)
    pr, lwr, ir = ref.sample_and_log_weights(eps0, na, nb, noise_r=nr)
    mk2, _, _ = _setup(hmc=hmc)
    a = mk2(adaptive_spec.Adaptive, resample_threshold=tau, ess_decay=0.7)
    pa, lwa, ia = a.sample_and_log_weights(eps0, na, nb, noise_r=nr, force_betas=ref.B_space)
    assert a.betas == [float(b) for b in ref.B_space] and len(a.decisions) == 3           # decisions 0, 1, 2 ran and were recorded
    if tau is not None:
        assert ref.trace.resampled == a.trace.resampled
        assert all(np.array_equal(u, v) for u, v in zip(ref.trace.ancestors, a.trace.ancestors))
    assert torch.equal(pr.x, pa.x) and torch.equal(pr.log_q, pa.log_q) and torch.equal(pr.log_p, pa.log_p)
    scale = max(1.0, float(lwr.abs().max()))
    assert float((lwr - lwa).abs().max()) <= 1e-6 * scale
    assert abs(ir.log_Z - ia.log_Z) <= 1e-6 * max(1.0, abs(ir.log_Z)) and abs(ir.ess_ais - ia.ess_ais) <= 1e-5


@pytest.mark.parametrize("seed", [0, 1])
def test_plateau_at_beta_one_leaves_the_weights_alone(seed):
    """M = 8, rho = 0.5: the schedule reaches 1 before the last step; the transitions that follow move the chains on the target
    and leave log_w untouched.  Measured with this spec (printed by the test): beta = 1 first at index 6 (seed 0) and 7 (seed 1) of
    the M + 2 = 10 entries."""
    M = 8
    mk, (eps0, na, nb, nr), _ = _setup(D=6, B=1024, M=M, seed=seed, p_target=True)
    a = mk(adaptive_spec.Adaptive, ess_decay=0.5)
    a.sample_and_log_weights(eps0, na, nb)
    b = a.betas
    first = b.index(1.0)
    print(f"seed {seed}: betas {[round(v, 4) for v in b]}  beta = 1 first at index {first}")
    assert len(b) == M + 2 and b[0] == 0.0 and b[-1] == 1.0 and all(u <= v for u, v in zip(b, b[1:]))
    assert first < M, "the plateau this test is about did not occur"
    for j in range(first, M + 1):                       # log_w_after[j]: after the increment of step j (beta_j -> beta_{j+1})
        assert torch.equal(a.log_w_after[j], a.log_w_after[first - 1])
    assert all(d.beta < 1.0 for d in a.decisions) and len(a.decisions) == first


def _log_z_errors(rho, tau=None, M=4, seeds=range(8)):
    out = []
    for seed in seeds:
        mk, (eps0, na, nb, nr), tg = _setup(D=6, B=1024, M=M, seed=seed, p_target=True)
        if rho is None:
            s = mk(smc_spec.SMC, resample_threshold=tau)
            _, _, info = s.sample_and_log_weights(eps0, na, nb, noise_r=nr)
        else:
            s = mk(adaptive_spec.Adaptive, resample_threshold=tau, ess_decay=rho)
            _, _, info = s.sample_and_log_weights(eps0, na, nb, noise_r=nr)
        out.append(info.log_Z - tg.log_Z)
    return np.asarray(out)


def test_log_z_estimator_against_the_exact_normaliser():
    """tests/test_smc_spec.py's setup: ManyWell-6 (exact log Z), AIS target p, seeded_oracle_flow(6, 4, 10, 3), B = 1024, M = 4, HMC
    L = 5 with step 0.2 and tuning off, seeds 0 .. 7, no resampling; error = log_Z_hat - log_Z.  The bound is four standard errors
    of the LINEAR schedule's mean over the same seeds: |mean error at rho = 0.7| <= 4 std_linear / sqrt(8).
    Measured with this spec (printed by the test): linear mean -0.202, std 0.354 (bound 0.50); rho = 0.7 mean +0.057, std 0.125;
    rho = 0.5 mean -0.169, std 0.182."""
    lin = _log_z_errors(None)
    a7 = _log_z_errors(0.7)
    a5 = _log_z_errors(0.5)
    std_lin = float(lin.std(ddof=1))
    print(f"log Z error, M = 4, no resampling: linear mean {lin.mean():+.3f} std {std_lin:.3f}; adaptive rho=0.7 mean "
          f"{a7.mean():+.3f} std {a7.std(ddof=1):.3f}; rho=0.5 mean {a5.mean():+.3f} std {a5.std(ddof=1):.3f}; "
          f"bound {4 * std_lin / math.sqrt(8):.3f}")
    assert np.isfinite(a7).all() and np.isfinite(a5).all()
    assert abs(a7.mean()) <= 4 * std_lin / math.sqrt(8), (a7.mean(), std_lin)


# ---- host side of the product's settings (no GPU, no library load: everything fires before any op is reached) --------------------
def _product(M=2, D=4, **kw):
    import fab_torch_amd as fa
    target = fa.ManyWellEnergy(D)
    hmc = fa.HamiltonianMonteCarlo(M, D, lambda x: x.sum(-1), target.log_prob, alpha=2.0, p_target=False)
    return fa, target, hmc, (lambda base, **k: fa.AnnealedImportanceSampler(base, target.log_prob, hmc, False, 2.0, M, **{**kw, **k}))


def test_custom_schedules_are_validated_and_become_b_space():
    from fab_torch_amd._ops import FabhipError
    _, _, _, mk = _product(M=2)
    for good in ([0.0, 0.1, 0.1, 1.0], np.array([0, 0.5, 0.75, 1.0]), torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=torch.float64),
                 (0, 1e-3, 0.2, 1)):
        ais = mk(None, distribution_spacing_type=good)
        assert ais.B_space.dtype == torch.float64 and ais.B_space.tolist() == [float(v) for v in good]
        assert ais._betas() == [float(v) for v in good] and not ais.adaptive
    bad = {"length": [0.0, 0.5, 1.0], "start": [0.1, 0.2, 0.3, 1.0], "end": [0.0, 0.2, 0.3, 0.9], "order": [0.0, 0.6, 0.5, 1.0],
           "nan": [0.0, float("nan"), 0.5, 1.0], "inf": [0.0, 0.5, float("inf"), 1.0], "ndim": [[0.0, 0.5, 0.7, 1.0]],
           "dtype": torch.tensor([0.0, 0.5, 0.7, 1.0]), "text": ["a", "b", "c", "d"]}
    for what, v in bad.items():
        with pytest.raises(FabhipError, match="distribution_spacing_type"):
            mk(None, distribution_spacing_type=v)
    with pytest.raises(Exception, match="distribution spacing incorrectly specified"):
        mk(None, distribution_spacing_type="cosine")                  # (an unknown name: the reference's own exception)
    lin = mk(None).B_space
    assert torch.equal(mk(None, distribution_spacing_type="adaptive").B_space, lin)      # the nominal value


def test_ess_decay_is_validated_and_inert_elsewhere():
    from fab_torch_amd._ops import FabhipError
    fa, target, hmc, mk = _product()
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), "0.7", None, True):
        with pytest.raises(FabhipError, match="ess_decay"):
            mk(None, distribution_spacing_type="adaptive", ess_decay=bad)
    ais = mk(None, distribution_spacing_type="adaptive")
    assert ais.ess_decay == 0.7 and ais.adaptive
    ais.ess_decay = 0.5
    assert ais.ess_decay == 0.5
    with pytest.raises(FabhipError, match="ess_decay"):
        ais.ess_decay = 2
    assert not mk(None, ess_decay=0.3).adaptive                         # inert for the other spacings


def test_fab_model_passes_the_settings_through():
    import fab_torch_amd as fa
    D, M = 4, 2
    target = fa.ManyWellEnergy(D)
    flow = fa.RealNVP(D, 2, 3)
    hmc = fa.HamiltonianMonteCarlo(M, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False)
    m = fa.FABModel(flow, target, M, transition_operator=hmc, ais_distribution_spacing="adaptive", ais_ess_decay=0.6)
    assert m.annealed_importance_sampler.adaptive and m.annealed_importance_sampler.ess_decay == 0.6
    m = fa.FABModel(flow, target, M, transition_operator=hmc, ais_distribution_spacing=[0.0, 0.2, 0.2, 1.0])
    assert m.annealed_importance_sampler.B_space.tolist() == [0.0, 0.2, 0.2, 1.0]
    assert m.annealed_importance_sampler.ess_decay == 0.7


def test_routes_without_an_adaptive_schedule_refuse_it_by_name():
    from fab_torch_amd._ops import FabhipError
    from fab_torch_amd.spline_flow import CircularCoupledRQSFlow
    from fab_torch_amd import parallel
    from fab_torch_amd.point import Point
    fa, target, hmc, mk = _product(distribution_spacing_type="adaptive")
    D = 4
    # the fused spline call
    spline = CircularCoupledRQSFlow.__new__(CircularCoupledRQSFlow)      # (the refusal looks at the type only)
    ais = mk(spline)
    for call in (lambda: ais.sample_and_log_weights(8), lambda: ais.run(8), lambda: ais.generate_eval_data(8, 8)):
        with pytest.raises(FabhipError, match="adaptive.*spline"):
            call()
    # a defensive-mixture base
    mix = fa.DefensiveMixtureDistribution.__new__(fa.DefensiveMixtureDistribution)
    ais = mk(mix)
    for call in (lambda: ais.sample_and_log_weights(8), lambda: ais.run(8)):
        with pytest.raises(FabhipError, match="adaptive.*DefensiveMixtureDistribution"):
            call()
    # the generic path (a plug-in base distribution)
    ais = mk(object())
    for call in (lambda: ais.sample_and_log_weights(8), lambda: ais.run(8), lambda: ais.generate_eval_data(8, 8)):
        with pytest.raises(FabhipError, match="adaptive.*generic"):
            call()
    # one transition of a fixed schedule
    z = torch.zeros(3)
    with pytest.raises(FabhipError, match="adaptive.*perform_transition"):
        ais.perform_transition(Point(torch.zeros(3, D), z, z), z, 1)
    # both sharded samplers
    for cls in (parallel.ShardedAIS, parallel.ShardedAnnealedImportanceSampler):
        with pytest.raises(FabhipError, match="adaptive.*sharded"):
            parallel.refuse_adaptive(cls.__name__, ais)
    with pytest.raises(FabhipError, match="adaptive.*sharded"):
        parallel.ShardedAIS(ais.sample_and_log_weights).sample_and_log_weights(8)
    parallel.refuse_adaptive("ShardedAIS", mk(None, distribution_spacing_type="linear"))
    # a schedule of the caller's passes all of these gates; force_betas belongs to the adaptive mode
    fixed = mk(None, distribution_spacing_type=[0.0, 0.3, 0.3, 1.0])
    fixed._refuse_adaptive_routes()
    with pytest.raises(FabhipError, match="force_betas"):
        fixed.run(8, force_betas=[0.0, 0.3, 0.3, 1.0])
