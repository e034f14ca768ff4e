"""CPU tests of the SMC mode's specification (tests/smc_spec.py) and of the host-side refusals of the product's setting.  No GPU."""
import math

import numpy as np
import pytest
import torch

from helpers import seeded_oracle_flow
from oracle import ais as oais, targets as otgt
from oracle.numerical import fixed_point_weights
import smc_spec


def _setup(D=6, B=64, M=3, seed=0, hmc=True, eps=0.2, p_target=False):
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


@pytest.mark.parametrize("hmc", [True, False])
def test_threshold_none_is_the_oracle_ais(hmc):
    mk, (eps0, na, nb, nr), _ = _setup(hmc=hmc)
    pa, lwa, ia = mk(oais.AIS).sample_and_log_weights(eps0, na, nb)
    mk2, _, _ = _setup(hmc=hmc)
    ps, lws, is_ = mk2(smc_spec.SMC, resample_threshold=None).sample_and_log_weights(eps0, na, nb, noise_r=nr)
    assert torch.equal(pa.x, ps.x) and torch.equal(lwa, lws) and torch.equal(pa.log_q, ps.log_q)
    assert torch.equal(pa.log_p, ps.log_p) and ia == is_


def test_threshold_zero_never_resamples_and_equals_ais():
    mk, (eps0, na, nb, nr), _ = _setup()
    pa, lwa, _ = mk(oais.AIS).sample_and_log_weights(eps0, na, nb)
    mk2, _, _ = _setup()
    s = mk2(smc_spec.SMC, resample_threshold=0.0)
    ps, lws, _ = s.sample_and_log_weights(eps0, na, nb, noise_r=nr)
    assert not any(s.trace.resampled) and torch.equal(pa.x, ps.x) and torch.equal(lwa, lws)


@pytest.mark.parametrize("n", [1, 7, 64, 1000])
@pytest.mark.parametrize("u", [0.0, 0.3, 0.999999])
def test_equal_weights_give_identity_ancestors(n, u):
    d = smc_spec.decide(np.full(n, -3.25, np.float32), 1.5, u)
    assert d.resampled and np.array_equal(d.ancestors, np.arange(n))
    assert abs(d.ess - 1.0) < 1e-12 and d.log_w_common == np.float32(-3.25)


def test_decision_arithmetic_and_degenerate_rows():
    lw = np.array([0.0, -1.0, np.nan, -np.inf, np.inf, -2.0], np.float32)
    W = fixed_point_weights(lw)
    assert W[2] == W[3] == W[4] == 0 and W[0] == 2 ** 36
    d = smc_spec.decide(lw, 1.5, 0.5)
    w = W.astype(np.float64)
    assert d.resampled and abs(d.ess - w.sum() ** 2 / (6 * (w ** 2).sum())) < 1e-12
    assert set(d.ancestors.tolist()) <= {0, 1, 5}                       # weight-0 rows are never an ancestor
    none = smc_spec.decide(np.full(5, np.nan, np.float32), 1.5, 0.5)
    assert not none.resampled and none.ess == 0.0 and np.array_equal(none.ancestors, np.arange(5))
    assert not smc_spec.decide(lw, 0.0, 0.5).resampled


def test_always_resampling_keeps_logsumexp():
    mk, (eps0, na, nb, nr), _ = _setup(B=256, M=4)
    nr = torch.rand(4, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    s = mk(smc_spec.SMC, resample_threshold=1.5)
    s.sample_and_log_weights(eps0, na, nb, noise_r=nr)
    assert all(s.trace.resampled)
    for pre, post in zip(s.trace.log_w_pre, s.trace.log_w_post):
        assert bool((post == post[0]).all())
        a, b = float(torch.logsumexp(pre.double(), 0)), float(torch.logsumexp(post.double(), 0))
        # float32 rounding of the common value + the relative 2e-6 of exp_spec
        assert abs(a - b) <= 4e-6 * max(1.0, abs(a)), (a, b)


def _log_z_errors(tau, seeds=range(8)):
    D, B, M = 6, 1024, 4
    out, n_res = [], 0
    for seed in seeds:
        mk, (eps0, na, nb, nr), tg = _setup(D=D, B=B, M=M, seed=seed, p_target=True)
        s = mk(smc_spec.SMC, resample_threshold=tau)
        _, _, info = s.sample_and_log_weights(eps0, na, nb, noise_r=nr)
        out.append(info.log_Z - tg.log_Z)
        n_res += sum(s.trace.resampled) if s.trace is not None else 0
    return np.asarray(out), n_res


def test_log_z_estimator_against_the_exact_normaliser():
    """ManyWell-6 (exact log Z), AIS target p (alpha = 2 is passed and unused), seeded_oracle_flow(6, 4, 10, 3), B = 1024, M = 4,
    HMC L = 5 with step 0.2 and tuning off, seeds 0 .. 7; error = log_Z_hat - log_Z.  The bound is four standard errors of the plain sampler's
    mean over the same seeds: |mean error with tau = 0.5| <= 4 std_off / sqrt(8).
    Measured with this spec (printed by the test): off mean -0.202, std 0.354 (bound 0.50); tau = 0.5 mean -0.135, std 0.229, 24 of
    32 steps resampled; tau = 1.5 mean -0.131, std 0.221."""
    off, _ = _log_z_errors(None)
    on, n_res = _log_z_errors(0.5)
    always, _ = _log_z_errors(1.5)
    std_off = float(off.std(ddof=1))
    print(f"log Z error: off mean {off.mean():+.3f} std {std_off:.3f}; tau=0.5 mean {on.mean():+.3f} std {on.std(ddof=1):.3f} "
          f"({n_res} of {8 * 4} steps resampled); tau=1.5 mean {always.mean():+.3f} std {always.std(ddof=1):.3f}")
    assert np.isfinite(on).all() and n_res > 0
    assert abs(on.mean()) <= 4 * std_off / math.sqrt(8), (on.mean(), std_off)


# ---- host-side refusals of the product's setting (no GPU, no library load: they fire before any op is reached) ------------------
def test_spline_and_sharded_samplers_refuse_the_setting():
    import fab_torch_amd as fa
    from fab_torch_amd._ops import FabhipError
    from fab_torch_amd.spline_flow import CircularCoupledRQSFlow
    from fab_torch_amd import parallel

    D, M = 4, 2
    target = fa.ManyWellEnergy(D)
    flow = CircularCoupledRQSFlow.__new__(CircularCoupledRQSFlow)      # (the refusal looks at the type only)
    hmc = fa.HamiltonianMonteCarlo(M, D, lambda x: x.sum(-1), target.log_prob, alpha=2.0, p_target=False)
    ais = fa.AnnealedImportanceSampler(flow, target.log_prob, hmc, False, 2.0, M, resample_threshold=0.5)
    assert ais.resample_threshold == 0.5
    with pytest.raises(FabhipError, match="resample_threshold"):
        ais.sample_and_log_weights(8)
    with pytest.raises(FabhipError, match="resample_threshold"):
        ais.run(8)
    ais.resample_threshold = None                                      # settable
    for cls in (parallel.ShardedAIS, parallel.ShardedAnnealedImportanceSampler):
        with pytest.raises(FabhipError, match="resample_threshold"):
            parallel.refuse_resampling(cls.__name__, 0.5)
    parallel.refuse_resampling("ShardedAIS", None)


@pytest.mark.parametrize("bad", ["shape", "dtype", "ndim"])
def test_noise_r_is_validated(bad):
    from fab_torch_amd.ais import check_noise_r
    from fab_torch_amd._ops import FabhipError
    M = 4
    t = {"shape": torch.zeros(M + 1, dtype=torch.float64), "dtype": torch.zeros(M, dtype=torch.float32),
         "ndim": torch.zeros(M, 1, dtype=torch.float64)}[bad]
    with pytest.raises(FabhipError, match="noise_r"):
        check_noise_r(t, M)
    check_noise_r(torch.rand(M, dtype=torch.float64), M)


def test_threshold_is_validated():
    import fab_torch_amd as fa
    from fab_torch_amd._ops import FabhipError
    target = fa.ManyWellEnergy(4)
    hmc = fa.HamiltonianMonteCarlo(2, 4, lambda x: x.sum(-1), target.log_prob, alpha=2.0, p_target=False)
    with pytest.raises(FabhipError, match="resample_threshold"):
        fa.AnnealedImportanceSampler(None, target.log_prob, hmc, False, 2.0, 2, resample_threshold=float("nan"))
    with pytest.raises(FabhipError, match="resample_threshold"):
        fa.AnnealedImportanceSampler(None, target.log_prob, hmc, False, 2.0, 2, resample_threshold="0.5")
