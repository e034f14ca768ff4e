"""The native GMM and ManyWell targets (csrc/target_device.h: target_tile) on every kernel route that calls them, against the
float64 restatement of tests/target_cases.py (cases and their conditions: asserted on the CPU by tests/test_target_cases.py).

Every other test of the suite evaluates the GMM at the reference's one configuration - one scale for every component and
coordinate, D = 2 - where a wrong scale index, a dropped half log determinant or a component loop that stops after its first
pass give the bits of the correct code; and ManyWell at a, b, c = -0.5, -6, 1 without a normalisation constant.  Here every
scale is distinct, D runs from 1 to 64 = FABHIP_MAX_DIM, n_mix from 1 to 64, rows sit near one component, between two, and far
out on both sides of the -1e4 mask.

ONE criterion: `helpers.close` at RTOL against float64 (5e-4 for grad_log_q, as test_gpu_hmc_mass.py), non-finite patterns
exactly equal (masked rows -inf, NaN where the reference has NaN).  Gradients of log p: a row may instead be within 4x the
float32 restatement's own error on that row (the stressed-flow row rule), on at most B / 8 rows per comparison; every use is
printed ("MEASURE ... rows by the 4x clause").  An accept decision may differ only inside the rounding band, within the case's cap.
"""
import pytest
import torch

import hmc_mass_cases as mc
import target_cases as tc
from helpers import close, worst, RTOL
from test_gpu_parity import hip_flow_from_oracle, DEV

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
import test_gpu_hmc_mass as thm                       # noqa: E402
from fab_torch_amd import _ops                        # noqa: E402

M = tc.M_CHAIN
BATCHES = (1, 15, 16, 17, 48)                         # ragged against ROWS = 16 on both sides, one row, three full tiles
_flows, _targets = {}, {}


def native_gmm(locs, scales):
    """fa.GMM holding the case's means and scales in its buffers"""
    n_mix, D = locs.shape
    t = fa.GMM(D, n_mix, 1.0, true_expectation_estimation_n_samples=1000, locs=locs, scales=scales).to(DEV)
    assert torch.equal(t.locs.cpu(), locs) and torch.equal(t.scales.cpu(), scales) and t.locs.is_contiguous()
    return t


class ManyWellWithNorm(fa.ManyWellEnergy):
    """ManyWell with the C ABI's `log_norm` handed through as given (the class knows log Z for the default wells only)."""

    def __init__(self, dim, abc, log_norm):
        super().__init__(dim, a=abc[0], b=abc[1], c=abc[2])
        self._log_norm = float(log_norm)

    def native_target(self):
        return _ops.TARGET_MANYWELL, [float(self._a), float(self._b), float(self._c), self._log_norm], None, None


def native_manywell(D, abc, which):
    if which == "zero":
        return fa.ManyWellEnergy(D, a=abc[0], b=abc[1], c=abc[2])
    if which == "log_Z" and abc == tc.DEFAULT_ABC:
        return fa.ManyWellEnergy(D, normalised=True)
    return ManyWellWithNorm(D, abc, tc.mw_log_norm(D, which))


def same_nonfinite(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.where(torch.isinf(a), a, torch.zeros_like(a)),
                                                                      torch.where(torch.isinf(b), b, torch.zeros_like(b)))


def grad_close(tag, a, b64, b32):
    """the gradient rule of this file; returns the number of rows that needed the 4x clause"""
    a, b64, b32 = a.double().cpu(), b64.double(), b32.double()
    assert same_nonfinite(a, b64), f"{tag}: non-finite pattern of the gradient differs"
    if a.numel() == 0 or not bool(torch.isfinite(b64).any()):
        return 0
    z = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)          # noqa: E731
    u, u32 = tc.grad_units(a, b64), tc.grad_units(b32, b64)
    beyond = u > 1
    fin = torch.isfinite(b64)
    within4 = (torch.where(fin, (z(a) - z(b64)).abs() <= 4 * (z(b32) - z(b64)).abs(), torch.ones_like(fin))).all(1)
    print(f"MEASURE {tag} | grad log p | HIP {float(u.max()):.2f} | fp32 statement {float(u32.max()):.2f} | rows by the 4x clause "
          f"{int(beyond.sum())}")
    assert not bool((beyond & ~within4).any()), \
        f"{tag}: gradient rows {(beyond & ~within4).nonzero().flatten().tolist()[:8]} are {float(u[beyond & ~within4].max()):.2f} tolerances off"
    assert int(beyond.sum()) <= a.shape[0] // 8, f"{tag}: {int(beyond.sum())} rows need the 4x clause, cap {a.shape[0] // 8}"
    return int(beyond.sum())


def direct(tag, target, st64, st32, x64):
    """k_target<true> and k_target<false> on the rows x64 against the statements"""
    x = x64.float().to(DEV).contiguous()
    lp_g, g = target.log_prob_and_grad(x)
    lp = target.log_prob(x)
    torch.cuda.synchronize()
    assert lp.shape == (x.shape[0],) and g.shape == x.shape
    assert torch.equal(lp.nan_to_num(nan=7.0), lp_g.nan_to_num(nan=7.0)) and torch.equal(torch.isnan(lp), torch.isnan(lp_g)), \
        f"{tag}: log p of k_target<true> and k_target<false> differ in their bits"
    lp64, g64 = st64.log_prob_and_grad(x64)
    lp32, g32 = st32.log_prob_and_grad(x64.float())
    assert same_nonfinite(lp, lp64), f"{tag}: non-finite pattern of log p: {lp.cpu().tolist()[:6]} vs {lp64.tolist()[:6]}"
    print(f"MEASURE {tag} | log p | HIP {worst(lp.cpu(), lp64):.2f} | fp32 statement {worst(lp32, lp64):.2f}")
    assert close(lp.cpu(), lp64), f"{tag}: log p is {worst(lp.cpu(), lp64):.2f} tolerances from float64"
    return grad_close(tag, g, g64, g32)


# ---- (a) direct evaluation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n_mix,reference", tc.all_gmm_cases())
def test_gmm_log_prob_and_gradient_on_every_group_and_batch(D, n_mix, reference):
    c = tc.gmm_case(D, n_mix, reference)
    target = native_gmm(c["locs"], c["scales"])
    used = 0
    for name in tc.GROUPS:
        for B in BATCHES:
            used += direct(f"a GMM ({D}, {n_mix}){' reference' if reference else ''} {name} B={B}", target, c["st64"], c["st32"],
                           c["rows"][name][:B])
    # the special rows alone, and in one tile with live and masked rows
    sp = c["rows"]["special"]
    direct(f"a GMM ({D}, {n_mix}) special", target, c["st64"], c["st32"], sp)
    mixed = torch.cat([c["rows"]["far"][:7], sp, c["rows"]["near"][:7]])
    direct(f"a GMM ({D}, {n_mix}) special among live and masked rows", target, c["st64"], c["st32"], mixed)
    lp = target.log_prob(sp.float().to(DEV)).cpu()
    assert torch.isnan(lp[0]) and lp[1] == -tc.INF and torch.isfinite(lp[2])
    print(f"MEASURE a GMM ({D}, {n_mix}) | rows by the 4x clause in all | {used}")


@pytest.mark.parametrize("D,n_mix", [(5, 3), (16, 33), (60, 50)])
def test_gmm_backward_against_float64_autograd_with_a_non_constant_grad_out(D, n_mix):
    """_TargetLogProb.backward: grad_out[:, None] * the gradient of the same launch, masked rows included"""
    c = tc.gmm_case(D, n_mix)
    target = native_gmm(c["locs"], c["scales"])
    for name in tc.GROUPS:
        x64 = c["rows"][name]
        coef = torch.linspace(-1.5, 2.5, x64.shape[0], dtype=torch.float64)
        x = x64.float().to(DEV).requires_grad_(True)
        lp = target.log_prob(x)
        assert lp.requires_grad
        (gx,) = torch.autograd.grad(lp, x, grad_outputs=coef.float().to(DEV))
        xo = x64.clone().requires_grad_(True)
        (go,) = torch.autograd.grad(tc.otgt.GMM(D, n_mix, locs=c["locs"].double(), scales=c["scales"].double()).log_prob(xo), xo,
                                    grad_outputs=coef)
        g32 = coef.float()[:, None] * c["st32"].log_prob_and_grad(x64.float())[1]
        grad_close(f"a backward ({D}, {n_mix}) {name}", gx, go, g32)


@pytest.mark.parametrize("D,abc,which", tc.all_manywell_cases())
def test_manywell_log_prob_and_gradient_with_every_argument(D, abc, which):
    target = native_manywell(D, abc, which)
    st64, st32 = tc.manywell_statement(D, abc, which), tc.manywell_statement(D, abc, which, torch.float32)
    rows = tc.manywell_rows(D)
    for name in ("wide", "modes"):
        for B in BATCHES:
            direct(f"f ManyWell {D} {abc} log_norm {which} {name} B={B}", target, st64, st32, rows[name][:B])
    direct(f"f ManyWell {D} {abc} log_norm {which} special", target, st64, st32, rows["special"])
    direct(f"f ManyWell {D} {abc} log_norm {which} special among others", target, st64, st32,
           torch.cat([rows["wide"][:5], rows["special"], rows["modes"][:6]]))


# ---- (b) host checks --------------------------------------------------------------------------------------------------------------
def _bad_buffers(locs, scales):
    """(what, locs, scales) that no op may launch with"""
    n, D = locs.shape
    dl, ds = locs.to(DEV), scales.to(DEV)
    return [("scales one column wider", dl, torch.ones(n, D + 1, device=DEV)),
            ("scales one row longer", dl, torch.ones(n + 1, D, device=DEV)),
            ("locs flat", dl.reshape(-1), ds),
            ("locs with another dim", torch.zeros(n, D + 1, device=DEV), torch.ones(n, D + 1, device=DEV)),
            ("scales in float64", dl, ds.double()),
            ("locs in float64", dl.double(), ds),
            ("scales on the CPU", dl, scales.clone()),
            ("locs on the CPU", locs.clone(), ds),
            ("scales not contiguous", dl, ds.T.contiguous().T),
            ("locs not contiguous", dl.T.contiguous().T, ds),
            ("n_mix = 0", torch.zeros(0, D, device=DEV), torch.ones(0, D, device=DEV))]


def test_wrong_gmm_buffers_are_refused_before_any_launch():
    D, K, nodes, B, n_mix = tc.T_SHAPES[0]
    c = tc.t_case(D, K, nodes, B, n_mix)
    hf = hip_flow(D, K, nodes, c)
    x = c["start"].x.float().to(DEV)
    for what, bl, bs in _bad_buffers(c["locs"], c["scales"]):
        assert what.endswith("not contiguous") == (not (bl.is_contiguous() and bs.is_contiguous()))
        target = native_gmm(c["locs"], c["scales"])
        target.locs, target.scales = bl, bs
        for with_grad in (True, False):
            with pytest.raises(RuntimeError, match="fabhip"):
                target._native_log_prob(x, with_grad=with_grad)
        # ... and on the transition kernels, which check where they fill their own argument structs: the point stays untouched
        hmc = thm.make_hmc(c, hf.log_prob, target.log_prob, c["mass"])
        pt = thm.device_point(c["start"])
        with pytest.raises(RuntimeError, match="fabhip"):
            hmc.transition(pt, 1, tc.BETA, noise_p=c["noise_p"].to(DEV), noise_e=c["noise_e"].to(DEV))
        met = fa.Metropolis(1, D, hf.log_prob, target.log_prob, n_updates=2, alpha=tc.ALPHA, p_target=False).to(DEV)
        pm = fa.Point(pt.x.clone(), pt.log_q.clone(), pt.log_p.clone())
        with pytest.raises(RuntimeError, match="fabhip"):
            met.transition(pm, 1, tc.BETA)
        with pytest.raises(RuntimeError, match="fabhip"):
            fa.create_point(x, hf, target, with_grad=True)
        torch.cuda.synchronize()
        assert torch.equal(pt.x.cpu(), c["start"].x.float()) and torch.equal(pm.x.cpu(), c["start"].x.float()), what


def test_manywell_with_an_odd_dimension_is_refused():
    with pytest.raises(AssertionError):
        fa.ManyWellEnergy(5)
    x = torch.zeros(4, 5, device=DEV)
    for with_grad in (True, False):
        with pytest.raises(RuntimeError, match="fabhip"):
            _ops.load().target_logp_grad(_ops.TARGET_MANYWELL, [-0.5, -6.0, 1.0, 0.0], None, None, x, with_grad)
    # the class knows log Z for the default wells only (double_well.py:97-101 raises too): no silent constant
    with pytest.raises(NotImplementedError):
        fa.ManyWellEnergy(6, normalised=True, a=0.7, b=-3.0, c=0.5).log_prob(torch.zeros(4, 6, device=DEV))


# ---- (c) one teacher-forced HMC transition on every route --------------------------------------------------------------------------
def hip_flow(D, K, nodes, c):
    """the HIP twin of the case's oracle flow, built once per oracle flow (two cases of one shape have their own seeds)"""
    key = id(c["nf"])
    if key not in _flows:
        _flows[key] = (c["nf"], thm.spline_hip(c) if K == mc.SPLINE else hip_flow_from_oracle(c["nf"]))
    return _flows[key][1]


def native_target_of(shape, c):
    """the native twin of the case's target, built once per case (a whole call has its own means)"""
    key = id(c["st64"])
    if key not in _targets:
        _targets[key] = (c["st64"], ManyWellWithNorm(shape[0], tc.MW_T_ARGS[:3], tc.MW_T_ARGS[3]) if shape[4] == tc.MW else
                         native_gmm(c["locs"], c["scales"]))
    return _targets[key][1]


def check(tag, c, out, lw, grad_q=True, may_leave=0):
    """test_gpu_hmc_mass.check (x, log_q, log_p, log_w at RTOL, grad_log_q at 5e-4, decisions inside the band within the cap) on a
    case without special rows, and grad_log_p under the gradient rule on the rows it compared."""
    differ, same = thm.check(tag, c, out, lw, grad=grad_q, may_leave=may_leave, special_rows=False)
    both = same & (c["cls32"] == c["cls64"])
    rest = same & ~both                                        # (no float32 figure for a row whose float32 decision differs)
    grad_close(tag, out.grad_log_p[both], c["o64"].grad_log_p[both], c["o32"].grad_log_p[both])
    assert close(out.grad_log_p[rest], c["o64"].grad_log_p[rest]), f"{tag}: grad_log_p"
    return differ


_sixteen = {}


def transition_on(shape, tile, r4):
    D, K, nodes, B, n_mix = shape
    c = tc.t_case(*shape)
    hf, target = hip_flow(D, K, nodes, c), native_target_of(shape, c)
    with _ops.option(_ops.OPT_TILE_SHAPE, tile), _ops.option(_ops.OPT_R4_STREAM, r4):
        hmc = thm.make_hmc(c, hf.log_prob, target.log_prob, c["mass"])
        assert hmc.is_native and hmc.max_grad == 1e3
        out, lw = thm.run_transition(c, hmc)
    return c, out, lw


def on_route(tag, shape, tile, r4):
    c, out, lw = transition_on(shape, tile, r4)
    check(tag, c, out, lw)
    if shape not in _sixteen:
        _sixteen[shape] = out if tile == 16 else transition_on(shape, 16, 2)[1]
    if tile != 16:                                             # the intended route ran: another summation order, other bits
        assert not torch.equal(out.log_q, _sixteen[shape].log_q), "the 16-chain kernel ran"


@pytest.mark.parametrize("D,K,nodes,B,n_mix,kind,tile,r4", thm._routes(tc.T_SHAPES, tc.T_TILES, kinds=("unit",)))
def test_hmc_transition_with_the_gmm_on_every_route(D, K, nodes, B, n_mix, kind, tile, r4):
    on_route(f"c D={D} K={K} W={D * nodes} n_mix={n_mix} tile {tile} r4 {r4}", (D, K, nodes, B, n_mix), tile, r4)


@pytest.mark.parametrize("tile", [16, 4])
def test_hmc_transition_with_other_wells_and_a_normalisation_constant(tile):
    """(f) ManyWell at (a, b, c) = (0.7, -3, 0.5) with log_norm = 3.25: the constant enters log p and the log-weight increment"""
    on_route(f"f ManyWell {tc.MW_T_ARGS} tile {tile}", tc.MW_T_SHAPE, tile, 2)


# ---- (d) Metropolis ---------------------------------------------------------------------------------------------------------------
def test_metropolis_transition_with_the_gmm():
    """metropolis_body: target_tile<false> on every proposal, 17 components (lane 0 takes two), D = 5"""
    c = tc.metropolis_case()
    D, K, nodes, B, n_mix = tc.METROPOLIS_SHAPE
    hf, target = hip_flow(D, K, nodes, c), native_gmm(c["locs"], c["scales"])
    met = fa.Metropolis(1, D, hf.log_prob, target.log_prob, n_updates=tc.N_UPDATES, alpha=tc.ALPHA, p_target=False,
                        max_step_size=c["step"], min_step_size=c["step"] / 2, eval_mode=True).to(DEV)
    assert met.is_native
    s = c["start3"]
    pt = fa.Point(*(t.float().to(DEV).contiguous() for t in (s.x, s.log_q, s.log_p)))
    lw = c["lw_in"].float().to(DEV)
    scalings = met.noise_scalings.clone()
    met.transition(pt, 1, tc.BETA, log_w=lw, beta_next=tc.BETA_NEXT, noise_x=c["noise_x"].to(DEV), noise_u=c["noise_u"].to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(met.noise_scalings, scalings)
    o64, o32 = c["o64"], c["o32"]
    differ = mc.tol_units(pt.x.cpu(), o64.x) > 1               # a chain that took another decision sits at another candidate
    assert not bool((differ & ~c["in_band"]).any()) and int(differ.sum()) <= c["cap"], differ.nonzero().flatten().tolist()
    same = ~differ
    for k, a, b32, b64 in (("x", pt.x.cpu(), o32.x, o64.x), ("log_q", pt.log_q.cpu(), o32.log_q, o64.log_q),
                           ("log_p", pt.log_p.cpu(), o32.log_p, o64.log_p), ("log_w", lw.cpu(), c["lw32"], c["lw64"])):
        print(f"MEASURE d Metropolis | {k} | HIP {worst(a[same], b64[same]):.2f} | fp32 oracle {worst(b32[same], b64[same]):.2f}")
        assert close(a[same], b64[same]), f"Metropolis: {k} is {worst(a[same], b64[same]):.2f} tolerances from float64"
    assert 0 < int((pt.x.cpu() != s.x.float()).any(1).sum()) < B


# ---- (e) whole calls --------------------------------------------------------------------------------------------------------------
def chain_samplers(c, shape, mix=False):
    D, K, nodes, B, n_mix = shape
    hf, target = hip_flow(D, K, nodes, c), native_target_of(shape, c)
    base = hf
    if mix:
        base = fa.DefensiveMixtureDistribution(hf).to(DEV)
        with torch.no_grad():
            base.loc.fill_(mc.MIX_LOC); base.log_scale.fill_(mc.MIX_LOG_SCALE); base.mixture_logit.fill_(mc.MIX_LOGIT)
        base.requires_grad_(False)
    hmc = thm.make_hmc(c, base.log_prob, target.log_prob, c["mass"], n_dist=M)
    return hmc, fa.AnnealedImportanceSampler(base, target.log_prob, hmc, False, tc.ALPHA, M)


def fused_call(c, shape, **kw):
    hmc, ais = chain_samplers(c, shape)
    pt, lw = ais.sample_and_log_weights(shape[3], eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV))
    return pt, lw


@pytest.mark.parametrize("shape,tile", [(tc.CHAIN_SHAPES[0], 4), (tc.CHAIN_SHAPES[0], 8), (tc.CHAIN_SHAPES[0], 16), (tc.CHAIN_SHAPES[1], 16)])
def test_whole_fused_call_with_the_gmm_against_the_oracle(shape, tile):
    """k_ais_init* and M = 3 transitions free-running, at M x RTOL as test_gpu_hmc_mass.test_whole_fused_call_against_the_oracle"""
    c = tc.chain_case(*shape)
    B = shape[3]
    with _ops.option(_ops.OPT_TILE_SHAPE, tile):
        pt, lw = fused_call(c, shape)
        if tile != 16:
            with _ops.option(_ops.OPT_TILE_SHAPE, 16):
                assert not torch.equal(fused_call(c, shape)[0].log_q, pt.log_q), "the 16-chain kernel ran"
    assert pt.x.shape[0] == B
    moved = thm.check_chain(f"e D={shape[0]} W={shape[0] * shape[2]} n_mix={shape[4]} tile {tile}", c, pt, lw)
    if bool(moved.any()):                                      # as there: the chain that left must come out bit for bit wherever it sits
        perm = torch.arange(B).flip(0)
        cp = dict(c, eps0=c["eps0"][perm], na=c["na"][:, :, perm].contiguous(), nb=c["nb"][:, :, perm].contiguous())
        with _ops.option(_ops.OPT_TILE_SHAPE, tile):
            pt_p, lw_p = fused_call(cp, shape)
        assert torch.equal(pt_p.x.cpu()[perm], pt.x.cpu()) and torch.equal(lw_p.cpu()[perm], lw.cpu())


def test_defensive_mixture_call_with_the_gmm():
    """k_hmc_step_mix (the MIX instantiation of the 16-chain body) through fabhip::ais_run_ext"""
    shape = tc.MIX_SHAPE
    c = tc.chain_case(*shape, mix=True)
    hmc, ais = chain_samplers(c, shape, mix=True)
    assert ais.is_native and not hmc.is_native
    pt, lw = ais.sample_and_log_weights(shape[3], eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV),
                                        sel=c["sel"].to(DEV))
    assert pt.x.shape[0] == shape[3]
    thm.check_chain("e defensive mixture with the GMM", c, pt, lw)


def test_spline_flow_transition_with_the_gmm(monkeypatch):
    """spline_r8.h's host tile (target_tile<true> on the moved point of every leapfrog) at D = 60 with 7 components, and the
    step-by-step path (k_target) bit for bit; against the oracle with the spline test's knot allowance and nothing else"""
    shape = tc.EXTRA_SHAPES[1]
    D, K, nodes, B, n_mix = shape
    c = tc.t_case(*shape)
    hf, target = hip_flow(D, K, nodes, c), native_target_of(shape, c)
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
    check("e spline D=60 with the GMM, host-fused", c, *outs["fused"], grad_q=False, may_leave=2)


def test_generic_path_with_the_native_gmm_as_its_log_prob_func():
    """k_gen_*: the base is a plug-in evaluated by torch, the target the native GMM (k_target<true> per leapfrog), D = 20"""
    shape = tc.EXTRA_SHAPES[0]
    D, K, nodes, B, n_mix = shape
    c = tc.t_case(*shape)
    base, target = mc.PlugGaussian(D), native_target_of(shape, c)
    hmc = thm.make_hmc(c, base.log_prob, target.log_prob, c["mass"])
    assert not hmc.is_native
    out, lw = thm.run_transition(c, hmc)
    check("e generic path D=20 with the GMM", c, out, lw)
