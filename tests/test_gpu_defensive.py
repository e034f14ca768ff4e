"""The defensive-mixture base distribution on the GPU (fab_torch_amd/defensive.py, csrc/defensive_device.h, the *_mix
instantiations of the 16-chain kernels) against its specification (tests/defensive_spec.py) in float64.

The fused-call cases (tests/defensive_cases.py) are chosen so that the float32 and the float64 spec agree on every accept
decision with a margin above 1e-3 (asserted on the CPU: tests/test_defensive_spec.py), so ALL chains are compared - a chain
whose decision differed would end at another point, far outside the tolerance.  Chains started on the Gaussian branch at
radius >= 40 (where the flow's float32 density is -inf) are among them; their values are orders of magnitude larger than the
others', so the two groups are compared separately (the absolute floor of `close` follows the largest entry).

Tolerances: rtol = RTOL = 1e-4 with the floors of tests/test_gpu_parity.py - atol_scale 10 for a gradient w.r.t. x, M for
quantities accumulated over the M transitions of a call, 30 for parameter gradients (sums over the batch)."""
import os

import numpy as np
import pytest
import torch

from helpers import close, worst, RTOL
import defensive_cases as dc
import defensive_spec as dspec
import smc_spec

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops, parallel     # noqa: E402
from oracle import flow as oflow             # noqa: E402

DEV = "cuda"


def hip_flow(nf, D, K, nodes, grad=False):
    f = fa.RealNVP(D, K, nodes)
    f._nf_model.load_state_dict({k: v.float() for k, v in nf.state_dict().items()})
    return f.to(DEV).requires_grad_(grad)


def hip_mixture(nf, D, K, nodes, loc=dc.LOC, log_scale=dc.LOG_SCALE, logit=dc.LOGIT, grad=False):
    m = fa.DefensiveMixtureDistribution(hip_flow(nf, D, K, nodes)).to(DEV)
    with torch.no_grad():
        m.loc.fill_(loc); m.log_scale.fill_(log_scale); m.mixture_logit.fill_(logit)
    return m.requires_grad_(grad)


def samplers(hmc, n_inner, p_target, base, tau=None, M=dc.M):
    target = fa.ManyWellEnergy(dc.D)
    alpha = None if p_target else 2.0
    if hmc:
        op = fa.HamiltonianMonteCarlo(M, dc.D, base.log_prob, target.log_prob, alpha=alpha, p_target=p_target, epsilon=dc.STEP,
                                      n_outer=n_inner, L=dc.L).to(DEV)
    else:
        op = fa.Metropolis(M, dc.D, base.log_prob, target.log_prob, n_updates=n_inner, alpha=alpha, p_target=p_target,
                           max_step_size=0.2, min_step_size=0.05).to(DEV)
    return op, fa.AnnealedImportanceSampler(base, target.log_prob, op, p_target, alpha, M, resample_threshold=tau)


_DEVICE_RUNS = {}


def device_run(case):
    """The fused call of one case on the GPU (once per session), tuning on, with the chains' starting points."""
    if case[0] not in _DEVICE_RUNS:
        name, hmc, n_inner, p_target, seed = case
        mix = hip_mixture(dc.flow(), dc.D, dc.K, dc.NODES)
        op, ais = samplers(hmc, n_inner, p_target, mix)
        assert ais.is_native and not op.is_native
        eps0, sel, na, nb = (t.to(DEV) for t in dc.inputs(hmc, n_inner, seed))
        pt, log_w, n_valid, stats, base_x, base_lw = ais.run(dc.B, eps0, na, nb, want_base=True, sel=sel)
        step = (op.epsilons.clone(), op.common_epsilon.clone()) if hmc else (op.noise_scalings.clone(),)
        _DEVICE_RUNS[case[0]] = dict(point=pt, log_w=log_w, n_valid=n_valid.cpu(), stats=stats.cpu(), base_x=base_x, base_lw=base_lw,
                                     step=step, mix=mix, eps0=eps0, sel=sel)
    return _DEVICE_RUNS[case[0]]


_SPEC_RUNS = {}


def spec_run(case):
    if case[0] not in _SPEC_RUNS:
        _SPEC_RUNS[case[0]] = dc.run_spec(case, torch.float64)
    return _SPEC_RUNS[case[0]]


def groups():
    far = torch.zeros(dc.B, dtype=torch.bool)
    far[list(dc.FAR_ROWS)] = True
    return (("far", far), ("near", ~far))


def assert_close_by_group(a, b, what, atol_scale=1.0):
    for tag, rows in groups():
        u, v = a.detach().cpu()[rows], b.detach().float()[rows]
        print(f"{what} [{tag}]: {worst(u, v):.3f} x tolerance (atol_scale 1)")
        assert close(u, v, RTOL, atol_scale=atol_scale), f"{what} [{tag}]: {worst(u, v):.2f} x tolerance"


# ---- 1. density and gradient kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K,W", [(2, 2, 16), (6, 2, 30), (32, 2, 64)])
def test_density_and_gradient_against_the_float64_spec(D, K, W):
    B, nodes = 37, W // D                                    # two full 16-row tiles and a ragged one
    torch.manual_seed(7)                                     # (the Linear layers' default initialisation)
    nf = oflow.make_realnvp(D, K, nodes)
    oflow.randomize_last_layers(nf, std=0.3, seed=7)
    x32 = dc.radius_rows(D, B, dtype=torch.float32)           # (last row: 1e20)
    x32[-2, 0] = float("nan")                                # and a row whose density is NaN by construction
    mix = hip_mixture(nf, D, K, nodes)
    lq, grad = mix.log_prob_and_grad(x32.to(DEV))
    lq_ng = mix.log_prob(x32.to(DEV))                        # the no-gradient instantiation: the same density
    assert close(lq_ng, lq, 1e-6), worst(lq_ng, lq, 1e-6)
    nf64 = nf.double()
    s64 = dspec.DefensiveMixture(nf64, torch.full((D,), dc.LOC), torch.full((D,), dc.LOG_SCALE), dc.LOGIT)
    lq64, g64, parts = dspec.log_prob_and_grad(nf64, s64.loc, s64.log_scale, s64.logit, x32.double())
    # float32 spec: which rows have a = -inf in float32 arithmetic, and what the 1e20 row gives
    s32 = dspec.DefensiveMixture(nf.float(), torch.full((D,), dc.LOC), torch.full((D,), dc.LOG_SCALE), dc.LOGIT)
    lq32, g32, parts32 = dspec.log_prob_and_grad(s32.nf, s32.loc, s32.log_scale, s32.logit, x32)
    body = slice(0, B - 2)
    r_f = parts["r_f"][body]
    # the three regimes: flow-dominated, mixed (the 3e-4 .. 0.99 of radii 2 and 4), a = -inf in float32
    assert float(r_f.max()) > 0.99 and bool(((r_f > 3e-4) & (r_f < 0.99)).any()) and bool(torch.isneginf(parts32["a"][body]).any())
    print(f"D={D}: log q {worst(lq[body], lq64[body].float()):.3f}, grad {worst(grad[body], g64[body].float()):.3f} x tolerance")
    assert bool(torch.isfinite(lq[body]).all()) and bool(torch.isfinite(grad[body]).all())
    assert close(lq[body], lq64[body].float(), RTOL), worst(lq[body], lq64[body].float())
    assert close(grad[body], g64[body].float(), RTOL, atol_scale=10), worst(grad[body], g64[body].float())
    # a NaN term gives NaN, as in the spec (the compaction removes such a row, as for a plain flow)
    assert bool(torch.isnan(lq64[-2])) and bool(torch.isnan(lq32[-2])) and bool(torch.isnan(lq[-2])) and bool(torch.isnan(lq_ng[-2]))
    # the row at 1e20: NaN, as in the spec, at D = 6 and D = 32 (the spec gives NaN there in float32 and in float64).  At D = 2
    # the spec itself gives no NaN (float32: -inf, float64: a finite -1.4e39, or NaN, with the CPU's exp) and the device's flow
    # gives -inf, for which the spec's formula is -inf (m = -inf): there the row is held to "never finite" and to the rule
    lq_flow_dev = mix.flow.log_prob(x32.to(DEV))
    assert not bool(torch.isfinite(lq[-1])) and not bool(torch.isfinite(lq_ng[-1]))
    if D != 2:
        assert bool(torch.isnan(lq32[-1])) and bool(torch.isnan(lq64[-1]))
        assert bool(torch.isnan(lq[-1])) and bool(torch.isnan(lq_ng[-1]))
    else:
        assert bool(torch.isnan(lq[-1])) == bool(torch.isnan(lq_flow_dev[-1]))
    print(f"D={D}: 1e20 row: device flow {float(lq_flow_dev[-1])}, mixture {float(lq[-1])}, spec f32 {float(lq32[-1])} f64 {float(lq64[-1])}")
    # rows whose flow density is -inf in float32: the gradient is the Gaussian term alone
    dead = torch.isneginf(lq_flow_dev).cpu()
    dead[-1] = dead[-2] = False
    assert int(dead.sum()) >= 1
    g_gauss = -(x32 - dc.LOC) * float(np.exp(np.float32(-2.0 * dc.LOG_SCALE)))
    assert close(grad.cpu()[dead], g_gauss[dead], 1e-6), worst(grad.cpu()[dead], g_gauss[dead], 1e-6)


# ---- 2. chain initialisation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [dc.CASES[0], dc.CASES[4]], ids=["hmc", "metropolis"])
def test_initialisation_branches_and_weights(case):
    name, hmc, n_inner, p_target, seed = case
    dev, spec = device_run(case), spec_run(case)
    assert int(dev["n_valid"][0]) == dc.B
    flow_rows = (dev["sel"] < torch.sigmoid(dev["mix"].mixture_logit.detach())).cpu()
    assert int((~flow_rows).sum()) == len(dc.FAR_ROWS) + len(dc.GAUSS_ROWS)
    # flow branch: bit-equal to the plain call's initialisation (16-chain tiles, the mixture's) for the same eps0
    plain_flow = dev["mix"].flow
    op, ais = samplers(hmc, n_inner, p_target, plain_flow)
    _, _, na, nb = (t.to(DEV) for t in dc.inputs(hmc, n_inner, seed))
    with _ops.option(_ops.OPT_TILE_SHAPE, 16):
        _, _, nv, _, plain_x0, _ = ais.run(dc.B, dev["eps0"], na, nb, want_base=True)
    assert int(nv[0]) == dc.B
    assert torch.equal(dev["base_x"][flow_rows.to(DEV)], plain_x0[flow_rows.to(DEV)])
    # Gaussian branch: loc + exp(log_scale) eps0
    # per element, 1e-6 relative to the magnitude of the two terms (the device differs by the rounding of expf and of the sum;
    # an element in which the terms cancel has no smaller absolute error than they have)
    step = torch.exp(torch.tensor(dc.LOG_SCALE)) * dev["eps0"].cpu()
    xg = dc.LOC + step
    err = (dev["base_x"].cpu()[~flow_rows] - xg[~flow_rows]).abs()
    assert bool((err <= 1e-6 * (abs(dc.LOC) + step[~flow_rows].abs())).all()), float((err / (abs(dc.LOC) + step[~flow_rows].abs())).max())
    assert all(float(dev["base_x"][r].norm()) >= 40.0 for r in dc.FAR_ROWS)
    assert_close_by_group(dev["base_x"], spec["x0"], "x0")
    # log p - log q0 of the starting points, log q0 being the mixture's density at x
    assert_close_by_group(dev["base_lw"], spec["base_log_w"], "base_log_w")
    if hmc:
        return
    # the initial log_w itself: a Metropolis call whose proposals are the current points (zero noise) leaves the chains where they
    # started, so its log_w is the initial one plus increments that depend on the starting point alone
    M1 = 1
    op, ais = samplers(False, 1, p_target, dev["mix"], M=M1)
    zeros_x, u = torch.zeros(M1, 1, dc.B, dc.D, device=DEV), torch.full((M1, 1, dc.B), 0.5, device=DEV)
    pt, log_w, nv, _, _, _ = ais.run(dc.B, dev["eps0"], zeros_x, u, sel=dev["sel"])
    assert int(nv[1]) == dc.B
    x0 = spec["x0"]
    lq0 = spec["mix"].log_prob(x0)
    from oracle import targets as otgt
    lp0 = otgt.ManyWell(dc.D).log_prob(x0)
    want = (2.0 * lp0 - lq0) - lq0                          # pi_1 = p^2 / q at beta = 1 (M = 1: betas 0, 1/2, 1), minus log q0
    assert_close_by_group(log_w, want, "log_w after a standing transition", atol_scale=2)


# ---- 3. the fused call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.CASES, ids=[c[0] for c in dc.CASES])
def test_fused_call_against_the_spec(case):
    name, hmc, n_inner, p_target, seed = case
    dev, spec = device_run(case), spec_run(case)
    assert tuple(int(v) for v in dev["n_valid"]) == (dc.B, dc.B) and spec["point"].x.shape[0] == dc.B
    pt, sp = dev["point"], spec["point"]
    # every accept decision equal: a chain that decided differently anywhere ends at another point
    assert_close_by_group(pt.x, sp.x, "x", atol_scale=dc.M)
    assert_close_by_group(pt.log_q, sp.log_q, "log_q", atol_scale=dc.M)
    assert_close_by_group(pt.log_p, sp.log_p, "log_p", atol_scale=dc.M)
    assert_close_by_group(dev["log_w"], spec["log_w"], "log_w", atol_scale=dc.M)
    if hmc:
        assert_close_by_group(pt.grad_log_q, sp.grad_log_q, "grad_log_q", atol_scale=10 * dc.M)
        assert_close_by_group(pt.grad_log_p, sp.grad_log_p, "grad_log_p", atol_scale=10 * dc.M)
        np.testing.assert_allclose(dev["step"][0].cpu().numpy(), spec["op"].epsilons.float().numpy(), rtol=1e-6)
        np.testing.assert_allclose(dev["step"][1].cpu().numpy(), spec["op"].common_epsilon.float().numpy(), rtol=1e-6)
        moved = (spec["op"].epsilons != dc.STEP * 0.9).any()
        assert bool(moved)
    else:
        np.testing.assert_allclose(dev["step"][0].cpu().numpy(), spec["op"].noise_scalings.float().numpy(), rtol=1e-6)
    st = dev["stats"]
    assert abs(float(st[3]) - spec["info"].ess_ais) <= 1e-3 * spec["info"].ess_ais + 1e-6
    assert abs(float(st[4]) - spec["info"].log_Z) <= 1e-4 * max(1.0, abs(spec["info"].log_Z))


# ---- 4. unchanged bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_mixture_off_is_the_plain_call_and_no_state_leaks(hmc):
    n_inner = 1 if hmc else 2
    eps0, sel, na, nb = (t.to(DEV) for t in dc.inputs(hmc, n_inner, 2))
    flow = hip_flow(dc.flow(), dc.D, dc.K, dc.NODES)
    mix = fa.DefensiveMixtureDistribution(flow).to(DEV).requires_grad_(False)
    ops = _ops.load()

    def plain_call(through_mix_op):
        op, ais = samplers(hmc, n_inner, False, flow)
        kind, slots = fa.ais.operator_slots(op)
        head = ais._call_head(flow, ais._native_parts()[1], kind)
        if through_mix_op:
            out = ops.ais_run_ext(*head, eps0, na, nb, *slots, True, 0, None, None, False, 0, *mix.mix_args(), None, False)
            assert all(t.numel() == 0 for t in out[10:])
            out = out[:10]
        else:
            out = ops.ais_run(*head, eps0, na, nb, *slots, True, 0)
        state = (op.epsilons.clone(), op.common_epsilon.clone()) if hmc else (op.noise_scalings.clone(),)
        return list(out), state

    with _ops.option(_ops.OPT_TILE_SHAPE, 16):
        a, sa = plain_call(False)
        b, sb = plain_call(True)
    assert all(torch.equal(u, v) for u, v in zip(a, b)), "ais_run_ext with mix_enabled = False differs from ais_run"
    assert all(torch.equal(u, v) for u, v in zip(sa, sb))
    # a plain sampler's result before and after a mixture call on the same flow (default tile choice: 4-chain tiles at B = 40)
    before, s0 = plain_call(False)
    op_m, ais_m = samplers(hmc, n_inner, False, mix)
    ais_m.run(dc.B, eps0, na, nb, sel=sel)
    after, s1 = plain_call(False)
    assert all(torch.equal(u, v) for u, v in zip(before, after)) and all(torch.equal(u, v) for u, v in zip(s0, s1))


# ---- 5. SMC mode + mixture, teacher-forced ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [1.5, 0.6])
def test_smc_decisions_with_the_mixture_equal_the_spec(tau):
    case = dc.CASES[0]
    name, hmc, n_inner, p_target, seed = case
    mix = hip_mixture(dc.flow(), dc.D, dc.K, dc.NODES)
    op, ais = samplers(hmc, n_inner, p_target, mix, tau=tau)
    eps0, sel, na, nb = (t.to(DEV) for t in dc.inputs(hmc, n_inner, seed))
    nr = torch.rand(dc.M, generator=torch.Generator().manual_seed(77), dtype=torch.float64)
    pt, log_w, n_valid, stats, _, _ = ais.run(dc.B, eps0, na, nb, noise_r=nr.to(DEV), trace=True, sel=sel)
    resampled, ess, anc, lw_pre = ais.last_smc
    n0 = int(n_valid[0])
    assert n0 == dc.B and anc.shape == (dc.M, dc.B)
    fired = 0
    for j in range(dc.M):
        d = smc_spec.decide(lw_pre[j][:n0].cpu().numpy(), tau, float(nr[j]))
        assert abs(d.ess - tau) >= 1e-3 * tau, f"transition {j + 1}: ess {d.ess} within 1e-3 of tau: a coin flip"
        assert bool(resampled[j]) == d.resampled and abs(float(ess[j]) - d.ess) <= 1e-6 * d.ess
        assert np.array_equal(anc[j].cpu().numpy().astype(np.int64)[:n0], d.ancestors), f"transition {j + 1}: ancestors differ"
        fired += d.resampled
    assert fired == dc.M if tau > 1 else fired >= 1
    # the weights the first decision saw are the mixture's initial log-weights
    spec = spec_run(case)
    lw0 = spec["ais"].snapshots[0][1]
    assert_close_by_group(lw_pre[0], lw0, "log_w_pre[0]")
    assert int(n_valid[1]) == dc.B and bool(torch.isfinite(log_w).all())


# ---- 6. parameter gradients of log_prob ---------------------------------------------------------------------------------------------
def test_parameter_gradients_of_log_prob():
    D, K, nodes, B = 6, 2, 5, 64
    torch.manual_seed(7)
    nf = oflow.make_realnvp(D, K, nodes)
    oflow.randomize_last_layers(nf, std=0.3, seed=7)
    g = torch.Generator().manual_seed(21)
    x32 = dc.radius_rows(D, B, seed=5, dtype=torch.float32)
    x32[-1] = torch.randn(D, generator=g)                    # (no NaN row here: a NaN density has no gradient to compare)
    coef = torch.randn(B, generator=g)
    mix = hip_mixture(nf, D, K, nodes, grad=True)
    lq = mix.log_prob(x32.to(DEV))
    assert lq.requires_grad
    (coef.to(DEV) * lq).sum().backward()
    assert bool(torch.isneginf(mix.flow.log_prob(x32.to(DEV)).detach()).any()), "rows with a dead flow term must be present"
    # float64 autograd of the spec's expression.  Rows whose flow term is -inf in float64 too take the Gaussian term alone, as
    # the spec says (r_f = 0) - the flow is not evaluated there, autograd through an infinite term being NaN; the flow term of
    # a row that is -inf in float32 only is ~ e^-100 here: negligible
    nf64 = nf.double()
    loc = torch.full((D,), dc.LOC, dtype=torch.float64, requires_grad=True)
    ls = torch.full((D,), dc.LOG_SCALE, dtype=torch.float64, requires_grad=True)
    lg = torch.tensor(dc.LOGIT, dtype=torch.float64, requires_grad=True)
    F = torch.nn.functional
    xd = x32.double()
    z = (xd - loc) * torch.exp(-ls)
    b = torch.sum(-0.5 * z * z - ls, 1) - 0.5 * D * np.log(2 * np.pi) + F.logsigmoid(-lg)
    with torch.no_grad():
        alive = torch.isfinite(nf64.log_prob(xd))
    assert int(alive.sum()) >= B // 2 and not bool(alive.all())
    a = nf64.log_prob(xd[alive]) + F.logsigmoid(lg)
    y = b.clone()
    y[alive] = torch.logsumexp(torch.stack((a, b[alive])), 0)
    assert close(lq.detach(), y.detach().float(), RTOL), worst(lq.detach(), y.detach().float())
    (coef.double() * y).sum().backward()
    want = dict(nf64.named_parameters())
    got = dict(mix.flow._nf_model.named_parameters())
    n_checked = 0
    for k, p in got.items():
        if k not in want:
            continue
        if want[k].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None and close(p.grad, want[k].grad.float(), RTOL, atol_scale=30), f"{k}: {worst(p.grad, want[k].grad.float()):.2f}"
        n_checked += 1
    assert n_checked >= 9 * K + 2
    for name, p, w in (("loc", mix.loc, loc), ("log_scale", mix.log_scale, ls), ("mixture_logit", mix.mixture_logit, lg)):
        print(name, worst(p.grad, w.grad.float()))
        assert close(p.grad, w.grad.float(), RTOL, atol_scale=30), f"{name}: {worst(p.grad, w.grad.float()):.2f}"


# ---- 7. trainer, evaluation, refusals -------------------------------------------------------------------------------------------------
def test_trainer_eval_and_refusals(tmp_path):
    D, K, nodes, M, B = 6, 2, 5, 2, 256
    torch.manual_seed(3)

    def build():
        flow = hip_flow(dc.flow(), D, K, nodes, grad=True)
        mix = fa.DefensiveMixtureDistribution(flow).to(DEV)
        target = fa.ManyWellEnergy(D)
        hmc = fa.HamiltonianMonteCarlo(M, D, mix.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.2, L=2).to(DEV)
        return mix, fa.FABModel(mix, target, M, alpha=2.0, transition_operator=hmc, loss_type="fab_alpha_div")
    mix, model = build()
    ais = model.annealed_importance_sampler
    assert ais.is_native
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)

    def init_sampler():
        pt, lw = ais.sample_and_log_weights(B, logging=False)
        return pt.x, lw, pt.log_q
    buf = fa.PrioritisedReplayBuffer(D, 4096, 512, init_sampler, device=DEV)
    trainer = fa.PrioritisedBufferTrainer(model, opt, buf, alpha=2.0, n_batches_buffer_sampling=2, max_gradient_norm=100.0,
                                          w_adjust_max_clip=10.0)
    start = {k: v.detach().clone() for k, v in mix.state_dict().items()}
    infos = [trainer.step(i + 1, B) for i in range(5)]
    assert all(np.isfinite(i["loss"]) for i in infos)
    end = mix.state_dict()
    for grp in ("loc", "log_scale", "mixture_logit"):
        assert not torch.equal(start[grp], end[grp]), f"{grp} did not move"
    assert any(not torch.equal(start[k], end[k]) for k in start if k.startswith("flow.") and k.endswith("weight"))
    # checkpoint round trip
    path = os.path.join(str(tmp_path), "model.pt")
    model.save(path)
    x = torch.randn(64, D, device=DEV) * 3.0
    with torch.no_grad():
        want = mix.log_prob(x)
    mix2, model2 = build()
    model2.load(path)
    with torch.no_grad():
        assert torch.equal(mix2.log_prob(x), want)
    info = model.get_eval_info(512, 256)
    assert np.isfinite(info["eval_ess_flow"]) and np.isfinite(info["eval_ess_ais"])
    # refusals
    with pytest.raises(_ops.FabhipError, match="DefensiveMixture"):
        parallel.ShardedAnnealedImportanceSampler(ais)
    mix.flow.precision = "fast"
    try:
        with pytest.raises(_ops.FabhipError, match="fp32"):
            ais.sample_and_log_weights(64)
        with pytest.raises(RuntimeError, match="fabhip"):      # and the library itself refuses the combination
            ops = _ops.load()
            kind, slots = fa.ais.operator_slots(ais.transition_operator)
            head = ais._call_head(mix.flow, ais._native_parts()[1], kind)
            ops.ais_run_ext(*head, torch.randn(64, D, device=DEV), None, None, *slots, False, _ops.PRECISION_FAST, None, None,
                            False, 0, *mix.mix_args(), None, True)
    finally:
        mix.flow.precision = None
