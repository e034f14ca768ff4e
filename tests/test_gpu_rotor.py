"""The native coupled-rotor target (FABHIP_TARGET_ROTOR: the fourth branch of csrc/target_device.h's target_tile) on every kernel
route that calls it, against the float64 restatement of tests/rotor_cases.py (the cases and their conditions are asserted on the
CPU by tests/test_rotor_cases.py).  The criterion is the one of test_gpu_targets.py: `helpers.close` at RTOL against float64 (5e-4
for grad_log_q), non-finite patterns exactly equal, its gradient rule for grad log p - and no row of a direct case may need that
rule's 4x clause - and, the cases having no accept decision inside the rounding band, no decision of a teacher-forced transition
may differ.  Whole calls run free: they keep test_gpu_hmc_mass.check_chain's rule and then ask for the same bits with the batch
reversed."""
import math

import numpy as np
import pytest
import torch

import hmc_mass_cases as mc
import rotor_cases as rc
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

M = rc.M_CHAIN
BATCHES = tgt.BATCHES
_flows, _targets = {}, {}


class RotorWithNorm(fa.CoupledRotorEnergy):
    """the C ABI's `log_norm` handed through as given (the class itself knows the constant without a coupling only)"""

    def __init__(self, c, log_norm):
        super().__init__(c["P"], c["A"], c["B"], c["K"], c["l"], c["q"])
        self._given_log_norm = float(log_norm)

    def native_target(self):
        kind, prm, T, S = super().native_target()
        return kind, prm[:3] + [self._given_log_norm], T, S


def native(c):
    """the native target holding the case's float32 rows and table bit for bit (and its log_norm), built once per case"""
    key = id(c["st64"])
    if key not in _targets:
        t = RotorWithNorm(c, c.get("log_norm", 0.0)).to(DEV)
        assert torch.equal(t.table.cpu(), c["table"]) and torch.equal(t.site_rows.cpu(), c["rows"])
        assert t.native_target()[0] == _ops.TARGET_ROTOR == 4 and t.table.is_contiguous() and t.site_rows.is_contiguous()
        _targets[key] = (c["st64"], t)
    return _targets[key][1]


def hip_flow(K, c):
    key = id(c["nf"])
    if key not in _flows:
        _flows[key] = (c["nf"], thm.spline_hip(c) if K == mc.SPLINE else hip_flow_from_oracle(c["nf"]))
    return _flows[key][1]


# ---- (a) direct evaluation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,density", rc.all_cases())
def test_log_prob_and_gradient_on_every_dimension_and_batch(D, density):
    c = rc.case(D, density)
    target = native(c)
    used = 0
    for B in BATCHES:
        used += tgt.direct(f"a rotor D={D} {density} NB={c['NB']} B={B}", target, c["st64"], c["st32"], c["rows_x"]["wide"][:B])
    sp = c["rows_x"]["special"]
    used += tgt.direct(f"a rotor D={D} {density} special", target, c["st64"], c["st32"], sp)
    used += tgt.direct(f"a rotor D={D} {density} special among others", target, c["st64"], c["st32"],
                       torch.cat([c["rows_x"]["wide"][:7], sp, c["rows_x"]["wide"][7:12]]))
    lp, g = target.log_prob_and_grad(sp.float().to(DEV))
    assert torch.isnan(lp[0]) and torch.isnan(lp[1]) and bool(torch.isnan(lp[2])) == c["has_line"]
    assert close(lp[3].cpu().double(), c["ref"]["special"][0][3]) and bool(torch.isfinite(g[3]).all())
    assert used == 0, "no row of these cases may need the 4x clause (test_rotor_cases.py: the float32 statement is inside a quarter)"
    # energy / force as CoupledQuarticEnergy has them
    x = c["rows_x"]["wide"][:5].float().to(DEV)
    assert torch.equal(target.energy(x), -target.log_prob(x)[:, None]) and torch.equal(target.force(x, 2.0), target.log_prob_and_grad(x)[1] / 2.0)


# ---- (b) backward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,density", [(15, "dense"), (33, "sparse"), (64, "dense")])
def test_backward_against_float64_autograd_with_a_non_constant_grad_out(D, density):
    c = rc.case(D, density)
    target = native(c)
    x64 = c["rows_x"]["wide"]
    coef = torch.linspace(-1.5, 2.5, x64.shape[0], dtype=torch.float64)
    x = x64.float().to(DEV).requires_grad_(True)
    lp = target.log_prob(x)
    assert lp.requires_grad
    (gx,) = torch.autograd.grad(lp, x, grad_outputs=coef.float().to(DEV))
    xo = x64.clone().requires_grad_(True)
    (go,) = torch.autograd.grad(rc.plain_log_prob(c["rows"], c["K32"], xo, rc.LOG_NORM), xo, grad_outputs=coef)
    g32 = coef.float()[:, None] * c["st32"].log_prob_and_grad(x64.float())[1]
    assert tgt.grad_close(f"b backward D={D} {density}", gx, go, g32) == 0


# ---- (c) exact periodicity -----------------------------------------------------------------------------------------------------------
def _grid_target(D=37):
    """periods 4 and 8 (rates 2^-2, 2^-3 exact), a few line sites, all three harmonics, a coupling with up to six neighbours"""
    g = torch.Generator().manual_seed(77)
    i = torch.arange(D)
    per = i % 5 != 4
    P = torch.where(per, torch.where(i % 2 == 0, 4.0, 8.0), 0.0).double()
    _, A, B, l, q = rc.draw_sites(D, g, periodic=per)
    K = rc.draw_coupling(P, g, "sparse")
    return fa.CoupledRotorEnergy(P, A, B, K, l, q).to(DEV), P, per


def test_log_prob_and_gradient_are_bit_identical_a_whole_number_of_periods_away():
    target, P, per = _grid_target()
    D = P.shape[0]
    g = torch.Generator().manual_seed(78)
    x = torch.randint(-4096, 4097, (48, D), generator=g).double() / 1024.0          # multiples of 2^-10 in [-4, 4]
    x[0, 0], x[1, 1], x[2, 2] = 2.0, 4.0, -2.0                                     # half a period: the tie of rint
    lp0, g0 = target.log_prob_and_grad(x.float().to(DEV))
    assert bool(torch.isfinite(lp0).all())
    for n in (-2, 1, 3):
        shift = n * P * (torch.rand(48, D, generator=g) < 0.7)                      # most periodic coordinates, not all
        y = (x + shift).float()
        assert torch.equal(y.double(), x + shift) and bool((shift[:, per] != 0).any())
        lp, gr = target.log_prob_and_grad(y.to(DEV))
        assert torch.equal(lp, lp0) and torch.equal(gr, g0), f"n = {n}: {int((lp != lp0).sum())} rows of log p differ"
        w = target.wrap(y.to(DEV))
        half = (0.5 * P).float().to(DEV)
        assert torch.equal(target.wrap(w), w) and bool((w[:, per] >= -half[per]).all() and (w[:, per] < half[per]).all())
        assert torch.equal(w[:, ~per], y.to(DEV)[:, ~per])
        assert torch.equal(target.log_prob(w), lp0)


# ---- (d) reductions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 17, 64])
def test_without_coupling_and_with_one_harmonic_it_is_the_von_mises_product(D):
    g = torch.Generator().manual_seed(80 + D)
    P = torch.empty(D, dtype=torch.float64).uniform_(2.0, 7.0, generator=g)
    A, B = (torch.empty(D, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g) for _ in range(2))
    t = fa.CoupledRotorEnergy(P, A, B, torch.zeros(D, D), normalised=True).to(DEV)
    x = ((torch.rand(48, D, generator=g, dtype=torch.float64) - 0.5) * 3 * P).float()
    vm = torch.distributions.VonMises(torch.atan2(B, A), torch.sqrt(A * A + B * B))
    th = 2 * math.pi * x.double() * t.site_rows[rc.ROW_RATE].cpu().double()         # (the rate as float32 holds it)
    want = (vm.log_prob(th) + torch.log(2 * math.pi / P)).sum(-1)
    lp = t.log_prob(x.to(DEV)).cpu()
    print(f"MEASURE d von Mises D={D} | log p | HIP {worst(lp, want):.2f}")
    assert close(lp, want), worst(lp, want)


@pytest.mark.parametrize("D", [1, 17, 64])
def test_on_line_only_sites_it_is_the_native_quartic_target(D):
    g = torch.Generator().manual_seed(90 + D)
    l = torch.empty(D, dtype=torch.float64).uniform_(-0.5, 0.5, generator=g)
    q = torch.empty(D, dtype=torch.float64).uniform_(0.2, 1.5, generator=g)
    z = torch.zeros(D, dtype=torch.float64)
    r = fa.CoupledRotorEnergy(z, z, z, torch.zeros(D, D), l, q, normalised=True).to(DEV)
    qt = fa.CoupledQuarticEnergy(l, q, z, torch.zeros(D, D), normalised=True).to(DEV)
    x = (torch.randn(48, D, generator=g) * 2).to(DEV)
    (lr, gr), (lq, gq) = r.log_prob_and_grad(x), qt.log_prob_and_grad(x)
    assert close(lr, lq.double()) and close(gr, gq.double()), (worst(lr.cpu(), lq.cpu().double()), worst(gr.cpu(), gq.cpu().double()))


@pytest.mark.parametrize("shape", rc.LATTICES)
def test_lattice_xy_is_the_loop_written_action(shape):
    J, field, period = 0.7, 0.3, 2 * math.pi if len(shape) != 2 else 3.0
    t = fa.LatticeXY(shape, J, field, period).to(DEV)
    D = int(np.prod(shape))
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(48, D, generator=g) * period).float()
    # the action at the angles the kernel sees: 2 pi x times the rate as float32 holds it
    rate = float(t.site_rows[rc.ROW_RATE, 0])
    S = rc.lattice_action(shape, J, field, 1.0 / rate, x)
    lp = t.log_prob(x.to(DEV)).cpu()
    print(f"MEASURE d LatticeXY {shape} | log p | HIP {worst(lp, -S):.2f}")
    assert close(lp, -S), worst(lp, -S)


# ---- (e) one teacher-forced HMC transition on every route -----------------------------------------------------------------------------
_sixteen = {}


def transition_on(shape, tile, r4):
    D, K, nodes, B = shape
    c = rc.t_case(*shape)
    hf, target = hip_flow(K, c), native(c)
    with _ops.option(_ops.OPT_TILE_SHAPE, tile), _ops.option(_ops.OPT_R4_STREAM, r4):
        hmc = thm.make_hmc(c, hf.log_prob, target.log_prob, c["mass"])
        assert hmc.is_native and hmc.max_grad == 1e3
        out, lw = thm.run_transition(c, hmc)
    return c, out, lw


@pytest.mark.parametrize("D,K,nodes,B,kind,tile,r4", thm._routes(rc.T_SHAPES, rc.T_TILES, kinds=("unit",)))
def test_hmc_transition_on_every_route(D, K, nodes, B, kind, tile, r4):
    shape = (D, K, nodes, B)
    c, out, lw = transition_on(shape, tile, r4)
    differ = tgt.check(f"e D={D} K={K} W={D * nodes} tile {tile} r4 {r4}", c, out, lw, may_leave=0)
    assert not bool(differ.any())
    if shape not in _sixteen:
        _sixteen[shape] = out if tile == 16 else transition_on(shape, 16, 2)[1]
    if tile != 16:                                             # the intended route ran: another summation order, other bits
        assert not torch.equal(out.log_q, _sixteen[shape].log_q), "the 16-chain kernel ran"


def test_metropolis_transition():
    """metropolis_body: target_tile<false> on every proposal, D = 5"""
    c = rc.metropolis_case()
    D, K, nodes, B = rc.METROPOLIS_SHAPE
    hf, target = hip_flow(K, c), native(c)
    met = fa.Metropolis(1, D, hf.log_prob, target.log_prob, n_updates=rc.N_UPDATES, alpha=rc.ALPHA, p_target=False,
                        max_step_size=c["step"], min_step_size=c["step"] / 2, eval_mode=True).to(DEV)
    assert met.is_native
    s = c["start3"]
    pt = fa.Point(*(t.float().to(DEV).contiguous() for t in (s.x, s.log_q, s.log_p)))
    lw = c["lw_in"].float().to(DEV)
    met.transition(pt, 1, rc.BETA, log_w=lw, beta_next=rc.BETA_NEXT, noise_x=c["noise_x"].to(DEV), noise_u=c["noise_u"].to(DEV))
    torch.cuda.synchronize()
    o64, o32 = c["o64"], c["o32"]
    for k, a, b32, b64 in (("x", pt.x.cpu(), o32.x, o64.x), ("log_q", pt.log_q.cpu(), o32.log_q, o64.log_q),
                           ("log_p", pt.log_p.cpu(), o32.log_p, o64.log_p), ("log_w", lw.cpu(), c["lw32"], c["lw64"])):
        print(f"MEASURE e Metropolis | {k} | HIP {worst(a, b64):.2f} | fp32 oracle {worst(b32, b64):.2f}")
        assert close(a, b64), f"Metropolis: {k} is {worst(a, b64):.2f} tolerances from float64"
    assert 0 < int((pt.x.cpu() != s.x.float()).any(1).sum()) < B


def test_spline_flow_transition_on_the_shared_torus(monkeypatch):
    """spline_r8.h's host tile (target_tile<true> on the moved point of every leapfrog) at D = 60 with the rotor target's periodic
    sites on the flow's circular coordinates, and the step-by-step path (k_target) bit for bit; against the oracle with the
    spline test's knot allowance and nothing else"""
    shape = rc.EXTRA_SHAPES[1]
    D, K, nodes, B = shape
    c = rc.t_case(*shape)
    hf, target = hip_flow(K, c), native(c)
    shared = fa.CoupledRotorEnergy.for_flow(hf, c["A"], c["B"], c["K"], c["l"], c["q"])
    assert torch.equal(shared.table.cpu(), c["table"]) and torch.equal(shared.site_rows.cpu(), c["rows"])
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
    tgt.check("e spline D=60, host-fused", c, *outs["fused"], grad_q=False, may_leave=2)


# ---- whole calls ---------------------------------------------------------------------------------------------------------------------
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
    return hmc, fa.AnnealedImportanceSampler(base, target.log_prob, hmc, False, rc.ALPHA, M)


def fused_call(c, shape):
    hmc, ais = chain_samplers(c, shape)
    assert ais.is_native
    return ais.sample_and_log_weights(shape[3], eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV))


def _reversed(c, B, with_sel=False):
    perm = torch.arange(B).flip(0)
    d = dict(c, eps0=c["eps0"][perm], na=c["na"][:, :, perm].contiguous(), nb=c["nb"][:, :, perm].contiguous())
    if with_sel:
        d["sel"] = c["sel"][perm]
    return d, perm


@pytest.mark.parametrize("shape,tile", [(rc.CHAIN_SHAPES[0], 4), (rc.CHAIN_SHAPES[0], 8), (rc.CHAIN_SHAPES[0], 16), (rc.CHAIN_SHAPES[1], 16)])
def test_whole_fused_call_against_the_oracle_and_with_the_batch_reversed(shape, tile):
    """k_ais_init* and M = 3 transitions free-running, at M x RTOL as test_gpu_hmc_mass.test_whole_fused_call_against_the_oracle;
    with the batch reversed every chain lands in another workgroup and lane and must come out bit for bit: an indexing error of the
    target (a site or a table column read for the wrong lane) moves with the position"""
    c = rc.chain_case(*shape)
    B = shape[3]
    with _ops.option(_ops.OPT_TILE_SHAPE, tile):
        pt, lw = fused_call(c, shape)
        if tile != 16:
            with _ops.option(_ops.OPT_TILE_SHAPE, 16):
                assert not torch.equal(fused_call(c, shape)[0].log_q, pt.log_q), "the 16-chain kernel ran"
        cp, perm = _reversed(c, B)
        pt_p, lw_p = fused_call(cp, shape)
    assert pt.x.shape[0] == B
    thm.check_chain(f"e call D={shape[0]} W={shape[0] * shape[2]} tile {tile}", c, pt, lw)
    assert torch.equal(pt_p.x.cpu()[perm], pt.x.cpu()) and torch.equal(lw_p.cpu()[perm], lw.cpu())


def test_defensive_mixture_call():
    """k_hmc_step_mix (the MIX instantiation of the 16-chain body) through fabhip::ais_run_ext"""
    shape = rc.MIX_SHAPE
    c = rc.chain_case(*shape, mix=True)
    hmc, ais = chain_samplers(c, shape, mix=True)
    assert ais.is_native and not hmc.is_native
    B = shape[3]
    call = lambda d: ais.sample_and_log_weights(B, eps0=d["eps0"].to(DEV), noise_a=d["na"].to(DEV), noise_b=d["nb"].to(DEV),      # noqa: E731
                                                sel=d["sel"].to(DEV))
    pt, lw = call(c)
    assert pt.x.shape[0] == B
    thm.check_chain("e defensive mixture", c, pt, lw)
    cp, perm = _reversed(c, B, with_sel=True)
    pt_p, lw_p = call(cp)
    assert torch.equal(pt_p.x.cpu()[perm], pt.x.cpu()) and torch.equal(lw_p.cpu()[perm], lw.cpu())


def test_one_rank_sharded_call_is_the_fused_call():
    """fabhip::ais_sharded_tuned on a one-rank gloo group: the sharded sampler hands native_target() through like the fused call,
    so with n_outer = 1 it gives that call's bits"""
    import datetime
    import os
    import torch.distributed as dist
    from fab_torch_amd import parallel
    shape = rc.CHAIN_SHAPES[0]
    D, K, nodes, B = shape
    c = rc.chain_case(*shape)
    hf, target = hip_flow(K, c), native(c)
    eps0, na, nb = c["eps0"].to(DEV), c["na"][:, :1].contiguous().to(DEV), c["nb"][:, :1].contiguous().to(DEV)

    def samplers():
        hmc = thm.make_hmc(c, hf.log_prob, target.log_prob, c["mass"], n_dist=M, tune=True, n_outer=1)
        return hmc, fa.AnnealedImportanceSampler(hf, target.log_prob, hmc, False, rc.ALPHA, M)
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


def test_fast_mode_keeps_the_target_in_float32():
    """fast mode rounds operands of the flow's inner GEMMs to bf16: x moves by up to a few 1e-3; log p and its gradient are
    float32 evaluations at the x the kernel arrived at"""
    shape = rc.T_SHAPES[2]
    c = rc.t_case(*shape)
    with fa.fast_mode():
        _, out, lw = transition_on(shape, 4, 2)
    _, ref, _ = transition_on(shape, 4, 2)
    assert not torch.equal(out.x, ref.x)
    lp64, g64 = c["st64"].log_prob_and_grad(out.x.double())
    lp32, g32 = c["st32"].log_prob_and_grad(out.x)
    assert close(out.log_p, lp64), worst(out.log_p, lp64)
    tgt.grad_close("e fast mode", out.grad_log_p, g64, g32)


def test_flow_move_with_the_rotor_target_equals_its_spec_bit_for_bit():
    """fabhip::flow_move (tests/flow_move_spec.py) with the rotor target behind create_point: the proposal's log p is the
    statement's, and the accepted rows are the spec's from the device's own densities"""
    import test_gpu_flow_moves as tfm
    shape = tfm.NARROW
    D, B = shape[0], 37
    g = torch.Generator().manual_seed(61)
    P, A, Bs, l, q = rc.draw_sites(D, g, amplitude=rc.T_AMPLITUDE)
    K = rc.draw_coupling(P, g, "dense")
    rows, table, _ = rc.pack(P, A, Bs, l, q, K)
    target = fa.CoupledRotorEnergy(P, A, Bs, K, l, q).to(DEV)
    flow = tfm._flow(shape)
    g0, gg = torch.randn(B, D, generator=g).to(DEV), torch.randn(B, D, generator=g).to(DEV)
    h = torch.empty(B).exponential_(1.0, generator=g).to(DEV)
    prop, start = tfm._proposal(flow, target, gg, True), tfm._proposal(flow, target, g0, True)
    lp64, g64 = rc.RotorStatement(rows, table).log_prob_and_grad(prop[0].cpu().double())
    assert close(prop[2].cpu(), lp64) and close(prop[4].cpu(), g64)
    seen = set()
    for beta in (0.3, 1.0):
        c_q, c_p = tfm.spec.anneal_coefs(beta, 2.0, False)
        cur = tuple(t.clone() for t in start)
        want = tfm.spec.move(tfm._np_point(start), tfm._np_point(prop), h.cpu().numpy(), c_q, c_p, B)
        frac, count = tfm._move_op(flow, target, cur, None, beta, 2.0, False, gg, h)
        tfm._assert_point_equals_spec(cur, want.point, f"beta={beta}")
        assert int(count) == want.n_accept
        seen.add(0 < want.n_accept < B)
    assert True in seen


# ---- LatticeXY: SMC mode and an adaptive schedule, against their specs on the device's own records --------------------------------------
LD, LK, LNODES, LM, LL, LSTEP, LB = 16, 3, 10, 4, 3, 0.05, 200


def lattice_samplers(**kw):
    nf = seeded_oracle_flow(LD, LK, LNODES, 7, std=0.01)
    hf = hip_flow_from_oracle(nf)
    target = fa.LatticeXY((4, 4), 1.2, field=0.2).to(DEV)
    op = fa.HamiltonianMonteCarlo(LM, LD, hf.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=LSTEP, L=LL,
                                  eval_mode=True).to(DEV)
    ais = fa.AnnealedImportanceSampler(hf, target.log_prob, op, False, 2.0, LM, **kw)
    st = rc.RotorStatement(target.site_rows.cpu(), target.table.cpu(), torch.float32)
    oop = oais.HMC(LM, LD, nf.log_prob, st.log_prob, alpha=2.0, p_target=False, epsilon=LSTEP, L=LL, eval_mode=True)
    spec = adaptive_spec.Adaptive(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, st.log_prob, oop, False, 2.0, LM,
                                  ess_decay=kw.get("ess_decay", 0.7), resample_threshold=kw.get("resample_threshold"))
    return ais, spec


def lattice_noise(seed):
    g = torch.Generator().manual_seed(300 + seed)
    return (torch.randn(LB, LD, generator=g), torch.randn(LM, 1, LB, LD, generator=g),
            torch.empty(LM, 1, LB).exponential_(1.0, generator=g), torch.rand(LM, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("mode", ["smc", "adaptive"])
def test_lattice_xy_in_smc_mode_and_on_an_adaptive_schedule(mode):
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
    assert 0.0 <= m["abs_magnetisation"] <= 1.0 and m["abs_magnetisation"] ** 2 <= m["magnetisation_sq"] + 1e-9
    assert -1.0 <= m["neighbour_cosine"] <= 1.0


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
def test_trainer_with_the_one_op_minibatch_step_on_the_lattice():
    """Three PrioritisedBufferTrainer iterations with every minibatch as ONE fabhip::buffer_train_step call on LatticeXY: finite
    losses; x is stored as added, a row no minibatch drew keeps log_w and log_q_old bit for bit, and with alpha = 2 log_w +
    log_q_old of a drawn row is what it was when the row was added (buffer.adjust's rule telescopes) - from the rows as the AIS
    calls with the rotor target handed them in"""
    Dt, Mt, B, NB, ALPHA = 16, 3, 256, 2, 2.0
    torch.manual_seed(1)
    flow = fa.make_wrapped_normflow_realnvp(Dt, 4, 10, act_norm=False).to(DEV)
    target = fa.LatticeXY((4, 4), 1.2, field=0.2).to(DEV)
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
        added.append((x.detach().clone(), log_w.detach().clone(), log_q_old.detach().clone()))
        plain_add(x, log_w, log_q_old)
    buf.add = recording_add
    while not buf.can_sample:
        buf.add(*initial_sampler())
    trainer = fa.PrioritisedBufferTrainer(model, fa.FlatAdam(flow, lr=1e-3), buf, alpha=ALPHA, n_batches_buffer_sampling=NB)
    assert trainer._fused and trainer._one_op_minibatch()            # every minibatch is ONE fabhip::buffer_train_step call
    drawn, n_iter = [], 3
    for i in range(n_iter):
        info = trainer.step(i, B)
        assert np.isfinite(info["loss"]), (i, info)
        drawn.append(trainer.last_indices.clone())
    torch.cuda.synchronize()
    n = buf.current_index
    assert n == (2 + n_iter) * B == sum(a[0].shape[0] for a in added) and not buf.is_full
    ax, alw, alq = (torch.cat([a[k] for a in added]) for k in range(3))
    sx, slw, slq = buf.buffer.x[:n], buf.buffer.log_w[:n], buf.buffer.log_q_old[:n]
    assert torch.isfinite(alw).all() and torch.isfinite(slw).all() and torch.equal(sx, ax)
    # the rows went in with the rotor target's log p: log_w = log p - log q at the end of an AIS call is not checked here (the
    # whole calls above do), but the target's value at the stored x is finite and periodic
    lp = target.log_prob(sx)
    assert bool(torch.isfinite(lp).all()) and close(target.log_prob(target.wrap(sx)).cpu(), lp.cpu().double(), 1e-4, atol_scale=8)
    touched = torch.zeros(n, dtype=torch.bool, device=DEV)
    touched[torch.cat(drawn)] = True
    assert 0 < int(touched.sum()) < n
    assert torch.equal(slw[~touched], alw[~touched]) and torch.equal(slq[~touched], alq[~touched])
    assert bool((slq[touched] != alq[touched]).any()), "the minibatch steps moved the parameters: log q of drawn rows changed"
    total, total_added = (slw + slq).double().cpu(), (alw + alq).double().cpu()
    assert close(total, total_added), worst(total, total_added)


# ---- (f) the constructor's refusals are test_rotor_cases.test_constructor_refuses_by_name (no GPU involved); on the device: ------------
def test_constructor_refusals_hold_on_the_device_too():
    D = 4
    P, A = torch.tensor([2.0, 3.0, 0.0, 4.0]), torch.tensor([0.5, 0.2, 0.0, -0.3])
    K = torch.zeros(D, D)
    K[0, 1] = K[1, 0] = 0.4
    l, q = torch.tensor([0.0, 0.0, 0.1, 0.0]), torch.tensor([0.0, 0.0, 0.5, 0.0])
    ok = fa.CoupledRotorEnergy(P.to(DEV), A.to(DEV), torch.zeros(D, device=DEV), K.to(DEV), l.to(DEV), q.to(DEV))
    assert ok.table.is_cuda and bool(torch.isfinite(ok.log_prob(torch.zeros(3, D, device=DEV))).all())
    Kn, Kd, Kl = K.clone(), K.clone(), K.clone()
    Kn[0, 3] = 0.2
    Kd[1, 1] = 0.1
    Kl[2, 3] = Kl[3, 2] = 0.1
    for match, args in (("not symmetric", (P, A, 0 * A, Kn, l, q)), ("non-zero diagonal", (P, A, 0 * A, Kd, l, q)),
                        ("touches a site on the line", (P, A, 0 * A, Kl, l, q)),
                        ("set on a periodic site", (P, A, 0 * A, K, l + 0.1, q)),
                        ("set on a site on the line", (P, A + 0.1, 0 * A, K, l, q)),
                        ("must be > 0 on a site on the line", (P, A, 0 * A, K, l, 0 * q)),
                        ("not finite", (P, A * float("nan"), 0 * A, K, l, q)),
                        ("above the 64", (torch.ones(65), torch.zeros(65), torch.zeros(65), torch.zeros(65, 65)))):
        with pytest.raises(ValueError, match=match):
            fa.CoupledRotorEnergy(*(a.to(DEV) for a in args))


# ---- (g) host checks ------------------------------------------------------------------------------------------------------------------
def _bad_buffers(T, S):
    D = T.shape[1]
    dt, ds = T.to(DEV), S.to(DEV)
    return [("site rows one column wider", dt, torch.ones(9, D + 1, device=DEV)),
            ("site rows with eight rows", dt, torch.ones(8, D, device=DEV)),
            ("site rows flat", dt, ds.reshape(-1)),
            ("table flat", dt.reshape(-1), ds),
            ("table with an odd number of rows", torch.zeros(3, D, device=DEV), ds),
            ("table one column wider", torch.zeros(2, D + 1, device=DEV), ds),
            ("table with NB = 0", torch.zeros(0, D, device=DEV), ds),
            ("table with NB = 64", torch.zeros(128, D, device=DEV), ds),
            ("site rows in float64", dt, ds.double()),
            ("table in float64", dt.double(), ds),
            ("site rows on the CPU", dt, S.clone()),
            ("table on the CPU", T.clone(), ds),
            ("site rows not contiguous", dt, ds.T.contiguous().T),
            ("table not contiguous", torch.zeros(T.shape[0], 2 * D, device=DEV)[:, ::2], ds)]


def test_wrong_buffers_are_refused_before_any_launch():
    shape = rc.T_SHAPES[0]
    D, K, nodes, B = shape
    c = rc.t_case(*shape)
    hf = hip_flow(K, c)
    x = c["start"].x.float().to(DEV)
    good = native(c)
    for what, bt, bs in _bad_buffers(good.table.cpu(), good.site_rows.cpu()):
        assert what.endswith("not contiguous") == (not (bt.is_contiguous() and bs.is_contiguous()))
        target = RotorWithNorm(c, 0.0).to(DEV)
        target.table, target.site_rows = bt, bs
        for with_grad in (True, False):
            with pytest.raises(RuntimeError, match="fabhip"):
                target._native_log_prob(x, with_grad=with_grad)
        hmc = thm.make_hmc(c, hf.log_prob, target.log_prob, c["mass"])
        pt = thm.device_point(c["start"])
        with pytest.raises(RuntimeError, match="fabhip"):
            hmc.transition(pt, 1, rc.BETA, noise_p=c["noise_p"].to(DEV), noise_e=c["noise_e"].to(DEV))
        met = fa.Metropolis(1, D, hf.log_prob, target.log_prob, n_updates=2, alpha=rc.ALPHA, p_target=False).to(DEV)
        pm = fa.Point(pt.x.clone(), pt.log_q.clone(), pt.log_p.clone())
        with pytest.raises(RuntimeError, match="fabhip"):
            met.transition(pm, 1, rc.BETA)
        with pytest.raises(RuntimeError, match="fabhip"):
            fa.create_point(x, hf, target, with_grad=True)
        torch.cuda.synchronize()
        assert torch.equal(pt.x.cpu(), c["start"].x.float()) and torch.equal(pm.x.cpu(), c["start"].x.float()), what
    # by message: what the op layer names
    ops = _ops.load()
    T, S = good.table, good.site_rows
    for match, bt, bs in (("rotor site rows must be", T, torch.ones(8, D, device=DEV)),
                          ("rotor neighbour table must be", torch.zeros(3, D, device=DEV), S),
                          ("1 <= NB <= 63", torch.zeros(128, D, device=DEV), S), ("1 <= NB <= 63", torch.zeros(0, D, device=DEV), S),
                          ("rotor target needs the neighbour table", None, None)):
        with pytest.raises(RuntimeError, match=match):
            ops.target_logp_grad(_ops.TARGET_ROTOR, [0.0, 0.0, 0.0, 0.0], bt, bs, x, True)
    with pytest.raises(RuntimeError, match="1 <= dim <= 64"):
        ops.target_logp_grad(_ops.TARGET_ROTOR, [0.0, 0.0, 0.0, 0.0], torch.zeros(2, 65, device=DEV), torch.zeros(9, 65, device=DEV),
                             torch.zeros(2, 65, device=DEV), True)
