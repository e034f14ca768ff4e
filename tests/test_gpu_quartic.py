"""The native coupled-quartic target (FABHIP_TARGET_QUARTIC: the third branch of csrc/target_device.h's target_tile) on every
kernel route that calls it, against the float64 restatement of tests/quartic_cases.py (the cases and their conditions are asserted
on the CPU by tests/test_quartic_cases.py).  The criterion is the one of test_gpu_targets.py: `helpers.close` at RTOL against
float64 (5e-4 for grad_log_q), non-finite patterns exactly equal, its gradient rule for grad log p, and - the cases have no accept
decision inside the rounding band - no decision of a teacher-forced transition may differ.  Whole calls run free: they keep
test_gpu_hmc_mass.check_chain's rule (one chain may leave the oracle at a ReLU kink within rounding) and then ask for the same
bits with the batch reversed."""
import numpy as np
import pytest
import torch

import hmc_mass_cases as mc
import quartic_cases as qc
import target_cases as tc
from helpers import close, worst, seeded_oracle_flow, max_rel_err, RTOL
from test_gpu_parity import hip_flow_from_oracle, DEV

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
import adaptive_spec                                  # noqa: E402
import test_gpu_hmc_mass as thm                       # noqa: E402
import test_gpu_smc as tsmc                           # noqa: E402
import test_gpu_targets as tgt                        # noqa: E402
from fab_torch_amd import _ops                        # noqa: E402
from oracle import ais as oais                        # noqa: E402

M = qc.M_CHAIN
BATCHES = tgt.BATCHES
_flows, _targets = {}, {}


class QuarticWithNorm(fa.CoupledQuarticEnergy):
    """the C ABI's `log_norm` handed through as given (the class itself knows the constant of its two exact cases only)"""

    def __init__(self, a, b, c, J, log_norm):
        super().__init__(a, b, c, J)
        self._given_log_norm = float(log_norm)

    def native_target(self):
        kind, prm, J, S = super().native_target()
        return kind, prm[:3] + [self._given_log_norm], J, S


def native(c):
    """the native target holding the case's float32 coefficients bit for bit (and its log_norm), built once per case"""
    key = id(c["st64"])
    if key not in _targets:
        t = QuarticWithNorm(c["a"], c["b"], c["c"], c["J"], c.get("log_norm", 0.0)).to(DEV)
        assert torch.equal(t.coupling.cpu(), c["J"]) and torch.equal(t.site_coefs.cpu(), torch.stack([c["a"], c["b"], c["c"]]))
        assert t.native_target()[0] == _ops.TARGET_QUARTIC == 3 and t.coupling.is_contiguous()
        _targets[key] = (c["st64"], t)
    return _targets[key][1]


def hip_flow(K, c):
    key = id(c["nf"])
    if key not in _flows:
        _flows[key] = (c["nf"], thm.spline_hip(c) if K == mc.SPLINE else hip_flow_from_oracle(c["nf"]))
    return _flows[key][1]


# ---- (a) direct evaluation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", qc.DIMS)
def test_log_prob_and_gradient_on_every_dimension_and_batch(D):
    c = qc.case(D)
    target = native(c)
    used = 0
    for B in BATCHES:
        used += tgt.direct(f"a quartic D={D} B={B}", target, c["st64"], c["st32"], c["rows"]["wide"][:B])
    sp = c["rows"]["special"]
    tgt.direct(f"a quartic D={D} special", target, c["st64"], c["st32"], sp)
    tgt.direct(f"a quartic D={D} special among others", target, c["st64"], c["st32"],
               torch.cat([c["rows"]["wide"][:7], sp, c["rows"]["wide"][7:13]]))
    lp, g = target.log_prob_and_grad(sp.float().to(DEV))
    assert torch.isnan(lp[0]) and not torch.isfinite(lp[1]) and float(lp[2]) == -qc.LOG_NORM and bool(torch.isfinite(g[2]).all())
    assert used == 0, "no row of these cases may need the 4x clause (test_quartic_cases.py: the float32 statement is inside a quarter)"
    # energy / force as ManyWellEnergy has them
    x = c["rows"]["wide"][:5].float().to(DEV)
    assert torch.equal(target.energy(x), -target.log_prob(x)[:, None]) and torch.equal(target.force(x, 2.0), target.log_prob_and_grad(x)[1] / 2.0)


@pytest.mark.parametrize("D", [15, 33, 64])
def test_backward_against_float64_autograd_with_a_non_constant_grad_out(D):
    c = qc.case(D)
    target = native(c)
    x64 = c["rows"]["wide"]
    coef = torch.linspace(-1.5, 2.5, x64.shape[0], dtype=torch.float64)
    x = x64.float().to(DEV).requires_grad_(True)
    lp = target.log_prob(x)
    assert lp.requires_grad
    (gx,) = torch.autograd.grad(lp, x, grad_outputs=coef.float().to(DEV))
    xo = x64.clone().requires_grad_(True)
    (go,) = torch.autograd.grad(c["st64"].log_prob_and_grad(xo)[0], xo, grad_outputs=coef)
    g32 = coef.float()[:, None] * c["st32"].log_prob_and_grad(x64.float())[1]
    assert tgt.grad_close(f"a backward D={D}", gx, go, g32) == 0


@pytest.mark.parametrize("D", [2, 18, 64])
def test_without_coupling_it_is_the_native_manywell(D):
    a, b, cc, J = qc.manywell_form(D)
    q, mw = fa.CoupledQuarticEnergy(a, b, cc, J).to(DEV), fa.ManyWellEnergy(D)
    for name in ("wide", "modes"):
        x = tc.manywell_rows(D)[name].float().to(DEV)
        (lq, gq), (lm, gm) = q.log_prob_and_grad(x), mw.log_prob_and_grad(x)
        assert close(lq, lm.double()) and close(gq, gm.double()), (worst(lq.cpu(), lm.cpu().double()), worst(gq.cpu(), gm.cpu().double()))
    # ... and normalised with the constant of the independent sites
    qn = fa.CoupledQuarticEnergy(a, b, cc, J, normalised=True).to(DEV)
    x = tc.manywell_rows(D)["modes"].float().to(DEV)
    assert close(qn.log_prob(x), fa.ManyWellEnergy(D, normalised=True).log_prob(x).double())


# ---- (b) one teacher-forced HMC transition on every route -----------------------------------------------------------------------------
_sixteen = {}


def transition_on(shape, tile, r4):
    D, K, nodes, B = shape
    c = qc.t_case(*shape)
    hf, target = hip_flow(K, c), native(c)
    with _ops.option(_ops.OPT_TILE_SHAPE, tile), _ops.option(_ops.OPT_R4_STREAM, r4):
        hmc = thm.make_hmc(c, hf.log_prob, target.log_prob, c["mass"])
        assert hmc.is_native and hmc.max_grad == 1e3
        out, lw = thm.run_transition(c, hmc)
    return c, out, lw


@pytest.mark.parametrize("D,K,nodes,B,kind,tile,r4", thm._routes(qc.T_SHAPES, qc.T_TILES, kinds=("unit",)))
def test_hmc_transition_on_every_route(D, K, nodes, B, kind, tile, r4):
    shape = (D, K, nodes, B)
    c, out, lw = transition_on(shape, tile, r4)
    differ = tgt.check(f"b D={D} K={K} W={D * nodes} tile {tile} r4 {r4}", c, out, lw, may_leave=0)
    assert not bool(differ.any())
    if shape not in _sixteen:
        _sixteen[shape] = out if tile == 16 else transition_on(shape, 16, 2)[1]
    if tile != 16:                                             # the intended route ran: another summation order, other bits
        assert not torch.equal(out.log_q, _sixteen[shape].log_q), "the 16-chain kernel ran"


# ---- (c) Metropolis, create_point ----------------------------------------------------------------------------------------------------
def test_metropolis_transition():
    """metropolis_body: target_tile<false> on every proposal, D = 5"""
    c = qc.metropolis_case()
    D, K, nodes, B = qc.METROPOLIS_SHAPE
    hf, target = hip_flow(K, c), native(c)
    met = fa.Metropolis(1, D, hf.log_prob, target.log_prob, n_updates=qc.N_UPDATES, alpha=qc.ALPHA, p_target=False,
                        max_step_size=c["step"], min_step_size=c["step"] / 2, eval_mode=True).to(DEV)
    assert met.is_native
    s = c["start3"]
    pt = fa.Point(*(t.float().to(DEV).contiguous() for t in (s.x, s.log_q, s.log_p)))
    lw = c["lw_in"].float().to(DEV)
    met.transition(pt, 1, qc.BETA, log_w=lw, beta_next=qc.BETA_NEXT, noise_x=c["noise_x"].to(DEV), noise_u=c["noise_u"].to(DEV))
    torch.cuda.synchronize()
    o64, o32 = c["o64"], c["o32"]
    for k, a, b32, b64 in (("x", pt.x.cpu(), o32.x, o64.x), ("log_q", pt.log_q.cpu(), o32.log_q, o64.log_q),
                           ("log_p", pt.log_p.cpu(), o32.log_p, o64.log_p), ("log_w", lw.cpu(), c["lw32"], c["lw64"])):
        print(f"MEASURE c Metropolis | {k} | HIP {worst(a, b64):.2f} | fp32 oracle {worst(b32, b64):.2f}")
        assert close(a, b64), f"Metropolis: {k} is {worst(a, b64):.2f} tolerances from float64"
    assert 0 < int((pt.x.cpu() != s.x.float()).any(1).sum()) < B


@pytest.mark.parametrize("shape", [qc.T_SHAPES[0], qc.T_SHAPES[3]], ids=str)
def test_create_point(shape):
    D, K, nodes, B = shape
    c = qc.t_case(*shape)
    hf, target = hip_flow(K, c), native(c)
    s = c["start"]
    for with_grad in (True, False):
        pt = fa.create_point(s.x.float().to(DEV), hf, target, with_grad=with_grad)
        assert close(pt.log_q.cpu(), s.log_q) and close(pt.log_p.cpu(), s.log_p), worst(pt.log_p.cpu(), s.log_p)
        if with_grad:
            assert close(pt.grad_log_q.cpu(), s.grad_log_q, 5e-4)
            tgt.grad_close(f"c create_point D={D}", pt.grad_log_p, s.grad_log_p, c["st32"].log_prob_and_grad(s.x.float())[1])


# ---- (d) whole calls -----------------------------------------------------------------------------------------------------------------
def chain_samplers(c, shape, mix=False):
    D, K, nodes, B = shape
    hf, target = hip_flow(K, c), native(c)
    base = hf
    if mix:
        base = fa.DefensiveMixtureDistribution(hf).to(DEV)
        with torch.no_grad():
            base.loc.fill_(mc.MIX_LOC); base.log_scale.fill_(mc.MIX_LOG_SCALE); base.mixture_logit.fill_(mc.MIX_LOGIT)
        base.requires_grad_(False)
    hmc = thm.make_hmc(c, base.log_prob, target.log_prob, c["mass"], n_dist=M)
    return hmc, fa.AnnealedImportanceSampler(base, target.log_prob, hmc, False, qc.ALPHA, M)


def fused_call(c, shape):
    hmc, ais = chain_samplers(c, shape)
    assert ais.is_native
    return ais.sample_and_log_weights(shape[3], eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV))


@pytest.mark.parametrize("shape,tile", [(qc.CHAIN_SHAPES[0], 4), (qc.CHAIN_SHAPES[0], 8), (qc.CHAIN_SHAPES[0], 16), (qc.CHAIN_SHAPES[1], 16)])
def test_whole_fused_call_against_the_oracle(shape, tile):
    """k_ais_init* and M = 3 transitions free-running, at M x RTOL as test_gpu_hmc_mass.test_whole_fused_call_against_the_oracle"""
    c = qc.chain_case(*shape)
    with _ops.option(_ops.OPT_TILE_SHAPE, tile):
        pt, lw = fused_call(c, shape)
        if tile != 16:
            with _ops.option(_ops.OPT_TILE_SHAPE, 16):
                assert not torch.equal(fused_call(c, shape)[0].log_q, pt.log_q), "the 16-chain kernel ran"
    assert pt.x.shape[0] == shape[3]
    moved = thm.check_chain(f"d D={shape[0]} W={shape[0] * shape[2]} tile {tile}", c, pt, lw)
    if bool(moved.any()):
        # No decision of the case sits inside the band, so the one chain check_chain's rule lets go met a ReLU kink within rounding
        # on its trajectory: a property of its DATA under this tile's arithmetic.  With the batch reversed it lands in another
        # workgroup and lane and must come out bit for bit; an indexing error of the target (a site or a row of J read for the
        # wrong lane) moves with the position and fails here.
        B = shape[3]
        perm = torch.arange(B).flip(0)
        cp = dict(c, eps0=c["eps0"][perm], na=c["na"][:, :, perm].contiguous(), nb=c["nb"][:, :, perm].contiguous())
        with _ops.option(_ops.OPT_TILE_SHAPE, tile):
            pt_p, lw_p = fused_call(cp, shape)
        assert torch.equal(pt_p.x.cpu()[perm], pt.x.cpu()) and torch.equal(lw_p.cpu()[perm], lw.cpu())


def test_defensive_mixture_call():
    """k_hmc_step_mix (the MIX instantiation of the 16-chain body) through fabhip::ais_run_ext"""
    shape = qc.MIX_SHAPE
    c = qc.chain_case(*shape, mix=True)
    hmc, ais = chain_samplers(c, shape, mix=True)
    assert ais.is_native and not hmc.is_native
    B = shape[3]
    call = lambda d: ais.sample_and_log_weights(B, eps0=d["eps0"].to(DEV), noise_a=d["na"].to(DEV), noise_b=d["nb"].to(DEV),      # noqa: E731
                                                sel=d["sel"].to(DEV))
    pt, lw = call(c)
    assert pt.x.shape[0] == B
    if bool(thm.check_chain("d defensive mixture", c, pt, lw).any()):          # (as in the whole fused call above)
        perm = torch.arange(B).flip(0)
        pt_p, lw_p = call(dict(c, eps0=c["eps0"][perm], na=c["na"][:, :, perm].contiguous(), nb=c["nb"][:, :, perm].contiguous(),
                               sel=c["sel"][perm]))
        assert torch.equal(pt_p.x.cpu()[perm], pt.x.cpu()) and torch.equal(lw_p.cpu()[perm], lw.cpu())


def test_one_rank_sharded_call_is_the_fused_call():
    """fabhip::ais_sharded_tuned on a one-rank gloo group (test_gpu_hmc_mass.test_one_rank_sharded_op_fills_the_same_mass_fields):
    the sharded sampler hands native_target() through like the fused call, so with n_outer = 1 it gives that call's bits"""
    import datetime
    import os
    import torch.distributed as dist
    from fab_torch_amd import parallel
    shape = qc.CHAIN_SHAPES[0]
    D, K, nodes, B = shape
    c = qc.chain_case(*shape)
    hf, target = hip_flow(K, c), native(c)
    eps0, na, nb = c["eps0"].to(DEV), c["na"][:, :1].contiguous().to(DEV), c["nb"][:, :1].contiguous().to(DEV)

    def samplers():
        hmc = thm.make_hmc(c, hf.log_prob, target.log_prob, c["mass"], n_dist=M, tune=True, n_outer=1)
        return hmc, fa.AnnealedImportanceSampler(hf, target.log_prob, hmc, False, qc.ALPHA, M)
    hmc1, ais1 = samplers()
    pt, lw = ais1.sample_and_log_weights(B, eps0=eps0, noise_a=na, noise_b=nb)
    hmc2, ais2 = samplers()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(thm._free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1, timeout=datetime.timedelta(seconds=60))
    try:
        pt2, lw2, _ = parallel.HipShardBackend(ais2).run_tuned(B, None, eps0, na, nb)
    finally:
        dist.destroy_process_group()
    for a, b in ((pt2.x, pt.x), (pt2.log_q, pt.log_q), (pt2.log_p, pt.log_p), (lw2, lw), (hmc2.epsilons, hmc1.epsilons),
                 (hmc2.common_epsilon, hmc1.common_epsilon)):
        assert torch.equal(a, b)
    # ... and the target is in it: log p at the returned x is the statement's
    assert close(pt2.log_p.cpu(), c["st64"].log_prob(pt2.x.cpu().double()))


def test_spline_flow_transition_host_fused_and_stepwise(monkeypatch):
    """spline_r8.h's host tile (target_tile<true> on the moved point of every leapfrog) at D = 60 and the step-by-step path
    (k_target) bit for bit; against the oracle with the spline test's knot allowance and nothing else"""
    shape = qc.EXTRA_SHAPES[1]
    D, K, nodes, B = shape
    c = qc.t_case(*shape)
    hf, target = hip_flow(K, c), native(c)
    outs = {}
    for mode in ("fused", "stepwise"):
        if mode == "stepwise":
            monkeypatch.setattr(fa.HamiltonianMonteCarlo, "force_stepwise", True)
        hmc = thm.make_hmc(c, hf.log_prob, target.log_prob, c["mass"])
        assert not hmc.is_native and (hmc._spline_parts() is None) == (mode == "stepwise")
        outs[mode] = thm.run_transition(c, hmc)
    for k in ("x", "log_q", "log_p", "grad_log_q", "grad_log_p"):
        assert torch.equal(getattr(outs["fused"][0], k), getattr(outs["stepwise"][0], k)), k
    assert torch.equal(outs["fused"][1], outs["stepwise"][1])
    tgt.check("d spline D=60, host-fused", c, *outs["fused"], grad_q=False, may_leave=2)


def test_generic_path_with_the_native_target_as_its_log_prob_func():
    """k_gen_*: the base is a plug-in evaluated by torch, the target the native one (k_target<true> per leapfrog), D = 20"""
    shape = qc.EXTRA_SHAPES[0]
    D, K, nodes, B = shape
    c = qc.t_case(*shape)
    base, target = mc.PlugGaussian(D), native(c)
    hmc = thm.make_hmc(c, base.log_prob, target.log_prob, c["mass"])
    assert not hmc.is_native
    out, lw = thm.run_transition(c, hmc)
    assert not bool(tgt.check("d generic path D=20", c, out, lw).any())


def test_fast_mode_keeps_the_target_in_float32():
    """fast mode rounds operands of the flow's inner GEMMs to bf16: x moves by up to a few 1e-3; log p and its gradient are
    float32 evaluations at the x the kernel arrived at"""
    shape = qc.T_SHAPES[2]
    c = qc.t_case(*shape)
    with fa.fast_mode():
        _, out, lw = transition_on(shape, 4, 2)
    _, ref, _ = transition_on(shape, 4, 2)
    assert not torch.equal(out.x, ref.x)                       # (a chain may take another accept decision under bf16 rounding:
    #                                                             x is not compared with the fp32 run, the target is - at the kernel's x)
    lp64, g64 = c["st64"].log_prob_and_grad(out.x.double())
    lp32, g32 = c["st32"].log_prob_and_grad(out.x)
    assert close(out.log_p, lp64), worst(out.log_p, lp64)
    tgt.grad_close("d fast mode", out.grad_log_p, g64, g32)


# ---- (e) LatticePhi4: SMC mode and an adaptive schedule, against their specs on the device's own records -------------------------------
LD, LK, LNODES, LM, LL, LSTEP, LB = 16, 3, 10, 4, 3, 0.05, 200


def lattice_samplers(**kw):
    nf = seeded_oracle_flow(LD, LK, LNODES, 7, std=0.01)
    hf = hip_flow_from_oracle(nf)
    target = fa.LatticePhi4((4, 4), 0.3, 0.02).to(DEV)                   # broken phase (kappa above the mean-field 1 / 2d)
    op = fa.HamiltonianMonteCarlo(LM, LD, hf.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=LSTEP, L=LL,
                                  eval_mode=True).to(DEV)
    ais = fa.AnnealedImportanceSampler(hf, target.log_prob, op, False, 2.0, LM, **kw)
    st = qc.QuarticStatement(target._a64, target._b64, target._c64, target._J64, torch.float32)
    oop = oais.HMC(LM, LD, nf.log_prob, st.log_prob, alpha=2.0, p_target=False, epsilon=LSTEP, L=LL, eval_mode=True)
    spec = adaptive_spec.Adaptive(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, st.log_prob, oop, False, 2.0, LM,
                                  ess_decay=kw.get("ess_decay", 0.7), resample_threshold=kw.get("resample_threshold"))
    return ais, spec


def lattice_noise(seed):
    g = torch.Generator().manual_seed(300 + seed)
    return (torch.randn(LB, LD, generator=g), torch.randn(LM, 1, LB, LD, generator=g),
            torch.empty(LM, 1, LB).exponential_(1.0, generator=g), torch.rand(LM, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("mode", ["smc", "adaptive"])
def test_lattice_phi4_in_smc_mode_and_on_an_adaptive_schedule(mode):
    tau = 1.5 if mode == "smc" else None
    kw = dict(resample_threshold=tau) if mode == "smc" else dict(distribution_spacing_type="adaptive", ess_decay=0.7)
    ais, spec = lattice_samplers(**kw)
    assert ais.is_native
    eps0, na, nb, nr = lattice_noise(1)
    pt, log_w, n_valid, stats, _, _ = ais.run(LB, eps0.to(DEV), na.to(DEV), nb.to(DEV), trace=True,
                                              noise_r=nr.to(DEV) if tau is not None else None)
    n0 = int(n_valid[0])
    assert n0 == LB == int(n_valid[1])
    teacher = None
    if mode == "smc":
        resampled, ess, anc, lw_pre = ais.last_smc
        for j in range(LM):
            d = tsmc.check_decision(lw_pre[j], n0, tau, nr[j], anc[j], resampled[j], ess[j], f"transition {j + 1}")
            assert d.resampled
        teacher = [lw_pre[j][:n0].cpu().numpy() for j in range(LM)]
        betas = list(ais._betas())
    else:
        betas = ais.last_betas.tolist()
        for d in ais.last_adaptive:
            lw, lq, lp = (t[:n0].cpu().numpy() for t in d.inputs)
            want = adaptive_spec.next_beta(lw, lq, lp, d.beta, 2.0, False, 0.7)
            assert d.beta_next == want.beta_next, f"decision {d.step}: beta_next {d.beta_next} vs spec {want.beta_next}"
    assert len(betas) == LM + 2 and betas[0] == 0.0 and betas[-1] == 1.0
    ps, lws, info = spec.sample_and_log_weights(eps0, na, nb, noise_r=nr if tau is not None else None, force_betas=betas,
                                                teacher_log_w_pre=teacher)
    assert max_rel_err(pt.x[:n0], ps.x) <= RTOL, f"x err {max_rel_err(pt.x[:n0], ps.x):.2e}: an accept decision differs"
    assert close(pt.log_q[:n0], ps.log_q, RTOL) and close(pt.log_p[:n0], ps.log_p, RTOL)
    assert close(log_w[:n0], lws, RTOL, atol_scale=4), f"log_w err {max_rel_err(log_w[:n0], lws):.2e}"
    m = ais.target_log_prob.__self__.performance_metrics(pt.x[:n0], log_w[:n0])
    assert 0.0 <= m["positive_share"] <= 1.0 and m["abs_magnetisation"] ** 2 <= m["magnetisation_sq"] + 1e-9


# ---- (f) the trainer ------------------------------------------------------------------------------------------------------------------
def test_trainer_with_the_one_op_minibatch_step_on_the_lattice():
    """Three PrioritisedBufferTrainer iterations with every minibatch as ONE fabhip::buffer_train_step call: finite losses, and the
    buffer holds what the rule of `buffer.adjust` makes of the rows the AIS calls added (recorded as they went in):
      * x is stored as added; a row no minibatch drew keeps log_w and log_q_old bit for bit;
      * a row that minibatches drew had log_w moved by (1 - alpha)(log q_new - log_q_old) and log_q_old set to log q_new each
        time, so with alpha = 2 log_w + log_q_old is what it was when the row was added (the adjustments telescope);
      * the rows of the last iteration's FIRST minibatch hold log q under the parameters that iteration started with (the
        minibatch evaluates before it steps): recomputed with a flow restored from a snapshot of those parameters."""
    Dt, Mt, B, NB, ALPHA = 16, 3, 256, 2, 2.0
    torch.manual_seed(1)
    flow = fa.make_wrapped_normflow_realnvp(Dt, 4, 10, act_norm=False).to(DEV)
    target = fa.LatticePhi4((4, 4), 0.3, 0.02).to(DEV)
    hmc = fa.HamiltonianMonteCarlo(Mt, Dt, flow.log_prob, target.log_prob, alpha=ALPHA, p_target=False, epsilon=0.1, L=3).to(DEV)
    model = fa.FABModel(flow, target, Mt, alpha=ALPHA, transition_operator=hmc, loss_type="fab_alpha_div")
    ais = model.annealed_importance_sampler
    assert ais.is_native

    def initial_sampler():
        pt, lw = ais.sample_and_log_weights(B, logging=False)
        return pt.x, lw, pt.log_q
    buf = fa.PrioritisedReplayBuffer(Dt, 8 * B, 2 * B, initial_sampler, device=DEV, fill_buffer_during_init=False)
    added, plain_add = [], buf.add

    def recording_add(x, log_w, log_q_old):
        assert buf.current_index == sum(a[0].shape[0] for a in added)               # (no wrap-around: 5 B rows of 8 B)
        added.append((x.detach().clone(), log_w.detach().clone(), log_q_old.detach().clone()))
        plain_add(x, log_w, log_q_old)
    buf.add = recording_add
    while not buf.can_sample:
        buf.add(*initial_sampler())
    trainer = fa.PrioritisedBufferTrainer(model, fa.FlatAdam(flow, lr=1e-3), buf, alpha=ALPHA, n_batches_buffer_sampling=NB)
    assert trainer._fused and trainer._one_op_minibatch()            # every minibatch is ONE fabhip::buffer_train_step call
    drawn, n_iter = [], 3
    for i in range(n_iter):
        if i == n_iter - 1:
            before_last = {k: v.detach().clone() for k, v in flow.state_dict().items()}
        info = trainer.step(i, B)
        assert np.isfinite(info["loss"]), (i, info)
        assert trainer.last_indices.shape == (NB * B,) and trainer.last_indices.unique().numel() == NB * B
        drawn.append(trainer.last_indices.clone())
    torch.cuda.synchronize()
    n = buf.current_index
    assert n == (2 + n_iter) * B == sum(a[0].shape[0] for a in added) and not buf.is_full
    ax, alw, alq = (torch.cat([a[k] for a in added]) for k in range(3))
    sx, slw, slq = buf.buffer.x[:n], buf.buffer.log_w[:n], buf.buffer.log_q_old[:n]
    assert torch.isfinite(alw).all() and torch.isfinite(slw).all() and torch.equal(sx, ax)
    touched = torch.zeros(n, dtype=torch.bool, device=DEV)
    touched[torch.cat(drawn)] = True
    assert 0 < int(touched.sum()) < n
    assert torch.equal(slw[~touched], alw[~touched]) and torch.equal(slq[~touched], alq[~touched])
    assert bool((slq[touched] != alq[touched]).any()), "the minibatch steps moved the parameters: log q of drawn rows changed"
    total, total_added = (slw + slq).double().cpu(), (alw + alq).double().cpu()
    print(f"MEASURE f trainer | log_w + log_q_old of drawn rows | {worst(total[touched.cpu()], total_added[touched.cpu()]):.2f}")
    assert close(total, total_added), worst(total, total_added)
    # log_q_old of the last iteration's first minibatch: log q under the parameters that iteration started with
    first = torch.chunk(drawn[-1], NB)[0]
    old = fa.make_wrapped_normflow_realnvp(Dt, 4, 10, act_norm=False).to(DEV)
    old.load_state_dict(before_last)
    with torch.no_grad():
        lq_old, lq_now = old.requires_grad_(False).log_prob(sx[first]), flow.log_prob(sx[first])
    assert not close(lq_now.cpu(), lq_old.double().cpu()), "the last iteration moved the parameters"
    assert close(slq[first].cpu(), lq_old.double().cpu()), worst(slq[first].cpu(), lq_old.double().cpu())


# ---- (g) host checks ------------------------------------------------------------------------------------------------------------------
def _bad_buffers(J, S):
    D = J.shape[0]
    dj, ds = J.to(DEV), S.to(DEV)
    return [("site coefficients one column wider", dj, torch.ones(3, D + 1, device=DEV)),
            ("site coefficients with two rows", dj, torch.ones(2, D, device=DEV)),
            ("site coefficients flat", dj, ds.reshape(-1)),
            ("coupling flat", dj.reshape(-1), ds),
            ("coupling one row longer", torch.zeros(D + 1, D, device=DEV), ds),
            ("coupling one column wider", torch.zeros(D, D + 1, device=DEV), ds),
            ("site coefficients in float64", dj, ds.double()),
            ("coupling in float64", dj.double(), ds),
            ("site coefficients on the CPU", dj, S.clone()),
            ("coupling on the CPU", J.clone(), ds),
            ("site coefficients not contiguous", dj, ds.T.contiguous().T),
            ("coupling not contiguous", torch.zeros(D, 2 * D, device=DEV)[:, ::2], ds)]


def test_wrong_buffers_are_refused_before_any_launch():
    shape = qc.T_SHAPES[0]
    D, K, nodes, B = shape
    c = qc.t_case(*shape)
    hf = hip_flow(K, c)
    x = c["start"].x.float().to(DEV)
    good = native(c)
    for what, bj, bs in _bad_buffers(good.coupling.cpu(), good.site_coefs.cpu()):
        assert what.endswith("not contiguous") == (not (bj.is_contiguous() and bs.is_contiguous()))
        target = fa.CoupledQuarticEnergy(c["a"], c["b"], c["c"], c["J"]).to(DEV)
        target.coupling, target.site_coefs = bj, bs
        for with_grad in (True, False):
            with pytest.raises(RuntimeError, match="fabhip"):
                target._native_log_prob(x, with_grad=with_grad)
        hmc = thm.make_hmc(c, hf.log_prob, target.log_prob, c["mass"])
        pt = thm.device_point(c["start"])
        with pytest.raises(RuntimeError, match="fabhip"):
            hmc.transition(pt, 1, qc.BETA, noise_p=c["noise_p"].to(DEV), noise_e=c["noise_e"].to(DEV))
        met = fa.Metropolis(1, D, hf.log_prob, target.log_prob, n_updates=2, alpha=qc.ALPHA, p_target=False).to(DEV)
        pm = fa.Point(pt.x.clone(), pt.log_q.clone(), pt.log_p.clone())
        with pytest.raises(RuntimeError, match="fabhip"):
            met.transition(pm, 1, qc.BETA)
        with pytest.raises(RuntimeError, match="fabhip"):
            fa.create_point(x, hf, target, with_grad=True)
        torch.cuda.synchronize()
        assert torch.equal(pt.x.cpu(), c["start"].x.float()) and torch.equal(pm.x.cpu(), c["start"].x.float()), what
    # the C ABI's own check: the kind without its buffers
    for with_grad in (True, False):
        with pytest.raises(RuntimeError, match="fabhip"):
            _ops.load().target_logp_grad(_ops.TARGET_QUARTIC, [0.0, 0.0, 0.0, 0.0], None, None, x, with_grad)
