"""CPU checks of the defensive-mixture specification (tests/defensive_spec.py): against the reference class's recorded
densities (tests/golden/g19_defensive_mixture.npz, made by tests/golden/make_golden_defensive.py), against oracle.ais on the
plain flow, and the properties the GPU tests (tests/test_gpu_defensive.py) rely on."""
import math

import numpy as np
import pytest
import torch

from helpers import load_golden, oracle_flow_from_golden
import defensive_cases as dc
import defensive_spec as dspec
from oracle import ais as oais
from oracle import flow as oflow
from oracle import targets as otgt


@pytest.fixture(scope="module")
def g19():
    g = load_golden("g19_defensive_mixture.npz")
    nf = oracle_flow_from_golden(g).double()
    mix = dspec.DefensiveMixture(nf, torch.tensor(g["loc"]), torch.tensor(g["log_scale"]), float(g["mixture_logit"]))
    return g, nf, mix


def test_product_module_exists_and_keeps_the_reference_parameters():
    """Names, shapes and initial values of the reference's parameters; a user-supplied defensive_dist is refused."""
    import fab_torch_amd as fa
    f = fa.RealNVP(6, 2, 5)
    m = fa.DefensiveMixtureDistribution(f)
    sd = m.state_dict()
    assert {"loc", "log_scale", "mixture_logit"} <= set(sd) and all(k.startswith("flow.") for k in set(sd) - {"loc", "log_scale", "mixture_logit"})
    assert sd["loc"].shape == (6,) and sd["log_scale"].shape == (6,) and sd["mixture_logit"].shape == ()
    assert float(sd["loc"].abs().max()) == 0 and float(sd["log_scale"].abs().max()) == 0 and float(sd["mixture_logit"]) == 1.0
    assert m.event_shape == (6,) and len(list(m.parameters())) == len(list(f.parameters())) + 3
    with pytest.raises(NotImplementedError, match="Gaussian"):
        fa.DefensiveMixtureDistribution(f, defensive_dist=object())


def test_density_equals_the_reference_and_gradient_equals_autograd(g19):
    g, nf, mix = g19
    x = torch.tensor(g["x"])
    lq, grad = mix.log_prob_and_grad(x)
    ref = torch.tensor(g["log_prob"])
    assert torch.isfinite(ref).all()
    assert float((lq - ref).abs().max()) <= 1e-6, float((lq - ref).abs().max())
    # float64 autograd of the same expression, on rows where both terms are finite (all of them in float64)
    xg = x.clone().requires_grad_(True)
    F = torch.nn.functional
    z = (xg - mix.loc) * torch.exp(-mix.log_scale)
    b = torch.sum(-0.5 * z * z - mix.log_scale, 1) - 0.5 * x.shape[1] * math.log(2 * math.pi) + F.logsigmoid(-mix.logit)
    a = nf.log_prob(xg) + F.logsigmoid(mix.logit)
    fin = (torch.isfinite(a) & torch.isfinite(b)).detach()
    assert int(fin.sum()) >= 18
    y = torch.logsumexp(torch.stack((a, b)), 0)
    ga = torch.autograd.grad(y[fin].sum(), xg)[0]
    scale = ga[fin].abs().max().clamp(min=1.0)
    assert float((grad[fin] - ga[fin]).abs().max() / scale) <= 1e-10
    # the three regimes are all present: flow-dominated, mixed, flow negligible
    r_f = dspec.log_prob_and_grad(nf, mix.loc, mix.log_scale, mix.logit, x)[2]["r_f"]
    assert float(r_f.max()) > 0.99 and float(r_f.min()) < 1e-6 and bool(((r_f > 1e-3) & (r_f < 0.99)).any())


@pytest.mark.parametrize("hmc", [True, False])
def test_logit_40_and_sel_0_is_the_plain_flow(hmc):
    """With logit = 40 (sigmoid = 1 - 4e-18) and sel = 0 the spec's AIS call is oracle.ais.AIS on the plain flow."""
    D, M, B = 6, 3, 24
    nf = dc.flow(torch.float64)
    mix = dspec.DefensiveMixture(nf, torch.full((D,), 0.25), torch.full((D,), 1.0), 40.0)
    tgt = otgt.ManyWell(D)
    g = torch.Generator().manual_seed(5)
    eps0 = torch.randn(B, D, generator=g, dtype=torch.float64)
    n_inner = 1 if hmc else 2
    na = torch.randn(M, n_inner, B, D, generator=g, dtype=torch.float64)
    nb = (torch.empty(M, n_inner, B, dtype=torch.float64).exponential_(1.0, generator=g) if hmc
          else torch.rand(M, n_inner, B, generator=g, dtype=torch.float64))

    def op(lq_fn):
        if hmc:
            return dc.RecHMC(M, D, lq_fn, tgt.log_prob, alpha=2.0, p_target=False, epsilon=dc.STEP, L=2, dtype=torch.float64)
        return dc.RecMetropolis(M, D, lq_fn, tgt.log_prob, n_updates=2, alpha=2.0, p_target=False, max_step_size=0.2,
                                min_step_size=0.05, dtype=torch.float64)
    om, op_plain = op(mix.log_prob), op(nf.log_prob)
    a_mix = dspec.make_ais(mix, tgt.log_prob, om, False, 2.0, M, torch.zeros(B, dtype=torch.float64))
    a_plain = oais.AIS(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, tgt.log_prob, op_plain, False, 2.0, M)
    pm, lwm, _ = a_mix.sample_and_log_weights(eps0, na, nb)
    pp, lwp, _ = a_plain.sample_and_log_weights(eps0, na, nb)
    assert len(om.accepts) == len(op_plain.accepts) == M * n_inner
    assert all(torch.equal(u, v) for u, v in zip(om.accepts, op_plain.accepts))
    acc = torch.stack(op_plain.accepts).double().mean()
    assert 0.05 < float(acc) < 0.95, f"the masks must hold accepts and rejects (mean acceptance {float(acc)})"
    # samples: equal (the Gaussian term's weight, 4e-18 of the flow's, is below half an ulp of the flow's density)
    assert torch.equal(pm.x, pp.x)
    assert float((pm.log_q - pp.log_q).abs().max()) <= 1e-6 and float((lwm - lwp).abs().max()) <= 1e-6


def test_ancestors_with_smc_equal_the_plain_flow():
    """The same equivalence through the SMC mode: the resampling decisions and ancestors of tests/smc_spec.py are equal."""
    import smc_spec
    D, M, B = 6, 3, 24
    nf = dc.flow(torch.float64)
    mix = dspec.DefensiveMixture(nf, torch.full((D,), 0.25), torch.full((D,), 1.0), 40.0)
    tgt = otgt.ManyWell(D)
    g = torch.Generator().manual_seed(6)
    eps0 = torch.randn(B, D, generator=g, dtype=torch.float64)
    na = torch.randn(M, 1, B, D, generator=g, dtype=torch.float64)
    nb = torch.empty(M, 1, B, dtype=torch.float64).exponential_(1.0, generator=g)
    nr = torch.rand(M, generator=g, dtype=torch.float64)
    mk = lambda fn: oais.HMC(M, D, fn, tgt.log_prob, alpha=2.0, p_target=False, epsilon=dc.STEP, L=2, dtype=torch.float64)   # noqa: E731
    s_mix = dspec.make_ais(mix, tgt.log_prob, mk(mix.log_prob), False, 2.0, M, torch.zeros(B, dtype=torch.float64),
                           cls=smc_spec.SMC, resample_threshold=1.5)
    s_plain = smc_spec.SMC(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, tgt.log_prob, mk(nf.log_prob),
                           False, 2.0, M, resample_threshold=1.5)
    s_mix.sample_and_log_weights(eps0, na, nb, noise_r=nr)
    s_plain.sample_and_log_weights(eps0, na, nb, noise_r=nr)
    assert s_mix.trace.resampled == s_plain.trace.resampled == [True] * M
    assert all(np.array_equal(u, v) for u, v in zip(s_mix.trace.ancestors, s_plain.trace.ancestors))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_branch_rule_at_the_threshold(dtype):
    """Chain i takes the flow branch iff sel_i < sigmoid(l): checked one ulp on either side of the threshold."""
    nf = dc.flow(dtype)
    mix = dc.mixture(nf)
    p = torch.sigmoid(mix.logit)
    below, above = torch.nextafter(p, torch.zeros_like(p)), torch.nextafter(p, torch.ones_like(p))
    sel = torch.stack([below, p, above, torch.zeros_like(p)]).to(dtype)
    assert mix.flow_branch(sel).tolist() == [True, False, False, True]
    eps0 = torch.randn(4, dc.D, generator=torch.Generator().manual_seed(1)).to(dtype)
    x, lq0 = mix.sample_eps(eps0, sel)
    x_flow = nf.sample_eps(eps0)[0].detach()
    x_gauss = mix.loc + torch.exp(mix.log_scale) * eps0
    assert torch.equal(x[0], x_flow[0]) and torch.equal(x[3], x_flow[3])
    assert torch.equal(x[1], x_gauss[1]) and torch.equal(x[2], x_gauss[2])
    assert torch.equal(lq0, mix.log_prob(x))                   # log_q0 is the density at x from the density direction


def test_mixture_bounds_q_where_the_float32_flow_underflows():
    """make_realnvp(6, 2, 5), std 0.3, seed 7, loc 0.25, log_scale 1, logit 1, rows of norm 40 and 200: the flow's float32
    log q is -inf on at least one row, the mixture's is finite on all rows and so is its gradient."""
    D = 6
    torch.manual_seed(7)                                       # (the Linear layers' default initialisation)
    nf = oflow.make_realnvp(D, 2, 5)
    oflow.randomize_last_layers(nf, std=0.3, seed=7)
    mix = dspec.DefensiveMixture(nf, torch.full((D,), 0.25), torch.full((D,), 1.0), 1.0)
    g = torch.Generator().manual_seed(11)
    u = torch.randn(32, D, generator=g)
    u = u / u.norm(dim=1, keepdim=True)
    x = u * torch.tensor([40.0, 200.0]).repeat(16)[:, None]
    with torch.no_grad():
        lq_flow = nf.log_prob(x)
    assert lq_flow.dtype == torch.float32 and bool(torch.isneginf(lq_flow).any())
    lq, grad = mix.log_prob_and_grad(x)
    assert bool(torch.isfinite(lq).all()) and bool(torch.isfinite(grad).all())
    dead = torch.isneginf(lq_flow)
    g_gauss = -(x - mix.loc) * torch.exp(-2.0 * mix.log_scale)
    assert torch.equal(grad[dead], g_gauss[dead])              # r_f = 0: the Gaussian term alone
    # a NaN density stays NaN (the compaction removes such a row, as for a plain flow); m = -inf gives -inf, not NaN
    bad = x[:2].clone()
    bad[0, 0], bad[1, 3] = float("nan"), float("inf")
    with torch.no_grad():
        assert bool(torch.isnan(nf.log_prob(bad)).all())
    assert bool(torch.isnan(mix.log_prob(bad)).all())
    far = dspec.DefensiveMixture(nf, torch.zeros(D), torch.full((D,), -40.0), 1.0)
    assert bool(torch.isneginf(far.log_prob(x[dead][:1])).all())


@pytest.mark.parametrize("case", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_accept_margins_of_the_gpu_cases(case):
    """For the seeds the GPU parity tests use, the float32 and the float64 spec run agree on every accept decision and every
    decision sits more than 1e-3 from its threshold (|delta + noise_e| for HMC, |exp(delta) - u| for Metropolis), in both
    runs: the GPU test may then compare ALL chains.  The chains started at radius >= 40 are among them."""
    r32, r64 = dc.run_spec(case, torch.float32), dc.run_spec(case, torch.float64)
    n_steps = dc.M * case[2]
    assert len(r32["op"].accepts) == len(r64["op"].accepts) == len(r64["op"].margins) == n_steps
    assert r64["point"].x.shape[0] == dc.B, "no chain may be dropped in these cases"
    for s in range(n_steps):
        assert torch.equal(r32["op"].accepts[s], r64["op"].accepts[s]), f"step {s}: float32 and float64 decide differently"
        for r in (r32, r64):
            m = r["op"].margins[s]
            fin = torch.isfinite(m)
            assert float(m[fin].abs().min()) > 1e-3, f"step {s}: margin {float(m[fin].abs().min())}"
    acc = torch.stack(r64["op"].accepts).double().mean()
    assert 0.05 < float(acc) < 0.999, f"the decisions must be of both kinds (mean acceptance {float(acc)})"
    x0 = r64["x0"]
    assert all(float(x0[r].norm()) >= 40.0 for r in dc.FAR_ROWS)
