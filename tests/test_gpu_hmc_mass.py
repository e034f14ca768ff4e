"""Every HIP route of an HMC transition with a NON-UNIT mass vector and an ACTIVE gradient clamp, against the float64 oracle
(cases and their conditions: tests/hmc_mass_cases.py, asserted on the CPU by tests/test_hmc_mass_cases.py).

With mass = ones and max_grad = 1e3 - what every other test of the suite runs - p0 = noise * m, x += eps / m * p and
K = sum(p^2 / m) / 2 give the bits of any other convention, and the clamp never binds.  Here the mass is log-uniform in [0.3, 3]
with mass[j] != mass[j + 16] (or the scalar 2.5), 12 - 20 % of the grad U components sit at each of +-max_grad, and three rows
start with +inf / -inf / NaN in grad_log_p.

ONE criterion for every comparison with the oracle: `helpers.close` at RTOL against float64 for x, log_q, log_p and log_w, 5e-4
for grad_log_q (as test_gpu_hmc_shapes.py) on the rows whose accept decisions are the float64 oracle's; a decision may differ
only on a row whose float64 margin lies inside the rounding band of test_gpu_stressed_flow.py's transition, and on at most `cap`
rows per case - the number of rows the case has inside that band (0 or 1, asserted on the CPU).  The whole call of (c) compounds
M transitions: M x the tolerance, as test_gpu_parity's g16, and at most one chain may leave the oracle, as test_gpu_r4f_handover.py.

Lines starting with "MEASURE" give the worst error of the HIP result and of the float32 oracle in tolerance units."""
import copy
import os

import pytest
import torch

import hmc_mass_cases as mc
from helpers import close, worst, RTOL
from test_gpu_parity import hip_flow_from_oracle, DEV
from test_gpu_sharded import _free_port

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops, parallel      # noqa: E402

M = mc.M_CHAIN
_flows = {}


def hip_flow(D, K, nodes, B):
    """the HIP twin of the case's oracle flow, built once per session."""
    if (D, K, nodes) not in _flows:
        _flows[(D, K, nodes)] = hip_flow_from_oracle(mc.inputs(D, K, nodes, B)["nf"])
    return _flows[(D, K, nodes)]


def make_hmc(c, log_q, log_p, mass_init, n_dist=1, tune=False, target_p_accept=0.65, n_outer=mc.N_OUTER):
    hmc = fa.HamiltonianMonteCarlo(n_dist, c["mass"].shape[0], log_q, log_p, alpha=mc.ALPHA, p_target=False, epsilon=c["epsilon"],
                                   n_outer=n_outer, L=c["L"], mass_init=mass_init, max_grad=c["max_grad"],
                                   target_p_accept=target_p_accept, eval_mode=not tune).to(DEV)
    assert torch.equal(hmc.epsilons.cpu()[0, :1], c["eps"][0, :1]) and torch.equal(hmc.common_epsilon.cpu(), c["ceps"])
    want = c["mass"] if torch.is_tensor(mass_init) else torch.full_like(c["mass"], mc.SCALAR_MASS)
    assert torch.equal(hmc.mass_vector.cpu(), want)
    return hmc


def device_point(p64):
    return fa.Point(*(t.float().to(DEV).contiguous() for t in (p64.x, p64.log_q, p64.log_p, p64.grad_log_q, p64.grad_log_p)))


def run_transition(c, hmc, i=1):
    """the case's transition, teacher-forced from its start point: (Point, log_w) on the CPU."""
    pt = device_point(c["start"])
    lw = c["lw_in"].float().to(DEV)
    hmc.transition(pt, i, mc.BETA, log_w=lw, beta_next=mc.BETA_NEXT, noise_p=c["noise_p"].to(DEV), noise_e=c["noise_e"].to(DEV))
    torch.cuda.synchronize()
    return fa.Point(*(t.cpu() for t in (pt.x, pt.log_q, pt.log_p, pt.grad_log_q, pt.grad_log_p))), lw.cpu()


def classes(x, x_in, trace):
    """per row: which of (start, first proposal, second proposal) the result sits at (hmc_mass_cases.final_class)."""
    cand = torch.stack([x_in.double(), trace[0]["x"].double(), trace[1]["x"].double()])
    return (x.double()[None] - cand).abs().amax(2).argmin(0)


def check(tag, c, out, lw, grad=True, may_leave=0, special_rows=True):
    """the one criterion, against the float64 oracle of case `c`.  `may_leave` (the spline flow only): test_gpu_spline.py's
    transition test lets two chains differ in x (a coordinate within rounding of a spline knot lands in the neighbouring bin); up
    to that many rows beyond the tolerance in x are counted, printed and left out of the other comparisons.  `special_rows=False`:
    a case of another file without the +inf / -inf / NaN rows.  Returns (rows whose decision differs, rows compared)."""
    cls = classes(out.x, c["start"].x, c["h64"].trace)
    differ = cls != c["cls64"]
    outside = differ & ~c["in_band"]
    assert not bool(outside.any()), (f"{tag}: {int(outside.sum())} accept decisions differ from float64 outside the rounding band: rows "
                                     f"{outside.nonzero().flatten().tolist()[:8]}, margins {c['margins'][:, outside].tolist()}")
    assert int(differ.sum()) <= c["cap"], f"{tag}: {int(differ.sum())} decisions differ, the case has {c['cap']} rows inside the band"
    same = ~differ
    o64, o32 = c["o64"], c["o32"]
    if may_leave:
        u = mc.tol_units(out.x, o64.x)
        left = same & (u > 1)
        print(f"MEASURE {tag} | rows beyond the tolerance in x | {[(int(r), round(float(u[r]), 2)) for r in left.nonzero().flatten()]}")
        assert int(left.sum()) <= may_leave, f"{tag}: {int(left.sum())} rows beyond the tolerance in x"
        same = same & ~left
    same32 = same & (c["cls32"] == c["cls64"])
    quantities = [("x", out.x, o32.x, o64.x, RTOL), ("log_q", out.log_q, o32.log_q, o64.log_q, RTOL),
                  ("log_p", out.log_p, o32.log_p, o64.log_p, RTOL), ("log_w", lw, c["lw32"], c["lw64"], RTOL)]
    if grad:
        quantities.append(("grad_log_q", out.grad_log_q, o32.grad_log_q, o64.grad_log_q, 5e-4))
    for k, a, b32, b64, rtol in quantities:
        print(f"MEASURE {tag} | {k} | HIP {worst(a[same], b64[same], rtol):.2f} | fp32 oracle {worst(b32[same32], b64[same32], rtol):.2f}")
    for k, a, b32, b64, rtol in quantities:
        assert close(a[same], b64[same], rtol), f"{tag}: {k} is {worst(a[same], b64[same], rtol):.2f} tolerances from float64"
    # the special rows: whatever the kernel made of +inf / -inf / NaN, it is inside the tolerance of clamp-then-nan_to_num
    if special_rows:
        assert bool((~differ)[list(mc.SPECIAL_ROWS)].all()) and bool((cls[list(mc.SPECIAL_ROWS)] != 0).all())
    return differ, same


# ---- (a) one transition, teacher-forced, on every tile shape and 4-chain schedule ------------------------------------------------
def _routes(shapes=mc.SHAPES, tiles=mc.TILES, kinds=("vector", "scalar")):
    """every (shape..., kind, tile shape, 4-chain schedule) for which a kernel exists"""
    out = []
    for shape in shapes:
        for kind in kinds:
            for tile in tiles[tuple(shape[:3])]:
                for r4 in ((2, 0, 1) if tile == 4 else (2,)):          # fused stages (default) / staged / stream
                    out.append(tuple(shape) + (kind, tile, r4))
    return out


_sixteen = {}


def transition_on(D, K, nodes, B, kind, tile, r4, **kw):
    c = mc.case(D, K, nodes, B, kind)
    hf, target = hip_flow(D, K, nodes, B), fa.ManyWellEnergy(D)
    with _ops.option(_ops.OPT_TILE_SHAPE, tile), _ops.option(_ops.OPT_R4_STREAM, r4):
        hmc = make_hmc(c, hf.log_prob, target.log_prob, c["mass"] if kind == "vector" else mc.SCALAR_MASS, **kw)
        out, lw = run_transition(c, hmc)
    return c, hmc, out, lw


@pytest.mark.parametrize("D,K,nodes,B,kind,tile,r4", _routes())
def test_single_transition_on_every_route(D, K, nodes, B, kind, tile, r4):
    c, _, out, lw = transition_on(D, K, nodes, B, kind, tile, r4)
    check(f"a D={D} K={K} W={D * nodes} {kind} tile {tile} r4 {r4}", c, out, lw)
    key = (D, K, nodes, kind)
    if key not in _sixteen:
        _sixteen[key] = out if tile == 16 else transition_on(D, K, nodes, B, kind, 16, 2)[2]
    if tile != 16:                                             # the intended route ran: another summation order, other bits
        assert not torch.equal(out.log_q, _sixteen[key].log_q), "the 16-chain kernel ran"


# ---- (b) the step-size rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [mc.TARGET_LOW, mc.TARGET_HIGH], ids=["grow", "shrink"])
@pytest.mark.parametrize("D,K,nodes,B,tile", mc.TUNED)
def test_step_size_rule_with_the_target_below_and_above_the_acceptance_rate(D, K, nodes, B, tile, target):
    """Tuning on: the second outer step runs on the common step size the first one adapted.  epsilons / common_epsilon equal the
    float32 oracle's bit for bit whenever no decision differed from it (the project's rule for step sizes)."""
    c, hmc, out, lw = transition_on(D, K, nodes, B, "vector", tile, 2, tune=True, target_p_accept=target)
    t32, t64 = (mc.tuned(D, K, nodes, B, "vector", target, dt) for dt in (torch.float32, torch.float64))
    cls = classes(out.x, c["start"].x, t64["trace"])
    differ64 = cls != t64["cls"]
    assert not bool((differ64 & ~t64["in_band"]).any()) and int(differ64.sum()) <= t64["cap"]
    same = ~differ64
    assert close(out.x[same], t64["out"].x[same], RTOL), worst(out.x[same], t64["out"].x[same])
    assert close(out.log_q[same], t64["out"].log_q[same], RTOL) and close(out.log_p[same], t64["out"].log_p[same], RTOL)
    grew = bool((hmc.epsilons.cpu() > c["eps"]).all())
    assert grew == (target == mc.TARGET_LOW) and not torch.equal(hmc.common_epsilon.cpu(), c["ceps"])
    if bool((cls == t32["cls"]).all()):
        assert torch.equal(hmc.epsilons.cpu(), t32["epsilons"]) and torch.equal(hmc.common_epsilon.cpu(), t32["ceps"])
    else:
        print("a decision differs from the float32 oracle: step sizes not compared")


# ---- (c) the whole fused call and the other entry points that fill the kernel's mass fields --------------------------------------
def chain_samplers(c, D, K, nodes, B, tune=False, n_outer=mc.N_OUTER, tau=None, mix=False):
    hf, target = hip_flow(D, K, nodes, B), fa.ManyWellEnergy(D)
    base = hf
    if mix:
        base = fa.DefensiveMixtureDistribution(hf).to(DEV)
        with torch.no_grad():
            base.loc.fill_(mc.MIX_LOC); base.log_scale.fill_(mc.MIX_LOG_SCALE); base.mixture_logit.fill_(mc.MIX_LOGIT)
        base.requires_grad_(False)
    hmc = make_hmc(c, base.log_prob, target.log_prob, c["mass"], n_dist=M, tune=tune, n_outer=n_outer)
    return hmc, fa.AnnealedImportanceSampler(base, target.log_prob, hmc, False, mc.ALPHA, M, resample_threshold=tau)


def check_chain(tag, c, pt, lw):
    FR = M * RTOL
    x = pt.x.cpu()
    p64, p32 = c["pt64"], c["pt32"]
    fin = torch.isfinite(p64.x)
    scale = max(1.0, float(p64.x[fin].abs().max()))
    moved = ((x.double() - p64.x).abs() > FR * p64.x.abs() + 2e-6 * M * scale).any(1)
    # the rule of test_gpu_r4f_handover.py / test_gpu_hmc_shapes.py for a free-running call: one chain may leave the oracle (an
    # accept threshold or a ReLU kink within rounding; it then differs as a whole and is left out of the other comparisons)
    print(f"MEASURE {tag} | chains that left the oracle | {moved.nonzero().flatten().tolist()} | inside the band {c['in_band'].nonzero().flatten().tolist()}")
    for r in moved.nonzero().flatten().tolist():
        u = ((x[r].double() - p64.x[r]).abs() / (FR * p64.x[r].abs() + 2e-6 * M * scale)).max()
        print(f"MEASURE {tag} | row {r} | x {float(u):.2f} units, log_w {float(lw.cpu()[r]):.6f} vs {float(c['lw64'][r]):.6f} | "
              f"smallest |margin| / band {float((c['margins'][:, r].abs() / c['bands'][:, r]).min()):.1f}, decisions {c['dec64'][:, r].tolist()}")
    assert int(moved.sum()) <= 1, f"{tag}: rows {moved.nonzero().flatten().tolist()} left the oracle"
    ok = ~moved
    ok32 = ok & (c["dec32"] == c["dec64"]).all(0)
    for k, a, b32, b64, rtol in (("x", x, p32.x, p64.x, FR), ("log_q", pt.log_q.cpu(), p32.log_q, p64.log_q, FR),
                                 ("log_p", pt.log_p.cpu(), p32.log_p, p64.log_p, FR), ("log_w", lw.cpu(), c["lw32"], c["lw64"], FR),
                                 ("grad_log_q", pt.grad_log_q.cpu(), p32.grad_log_q, p64.grad_log_q, M * 5e-4)):
        print(f"MEASURE {tag} | {k} | HIP {worst(a[ok], b64[ok], rtol):.2f} | fp32 oracle {worst(b32[ok32], b64[ok32], rtol):.2f}")
        assert close(a[ok], b64[ok], rtol, atol_scale=M), f"{tag}: {k} is {worst(a[ok], b64[ok], rtol):.2f} tolerances from float64"
    return moved


def fused_call(c, D, K, nodes, B, **kw):
    hmc, ais = chain_samplers(c, D, K, nodes, B, **kw)
    pt, lw = ais.sample_and_log_weights(B, eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV))
    return hmc, ais, pt, lw


@pytest.mark.parametrize("D,K,nodes,B,tile", [(32, 10, 10, 37, 4), (32, 10, 10, 37, 8), (32, 10, 10, 37, 16), (60, 2, 4, 20, 16)])
def test_whole_fused_call_against_the_oracle(D, K, nodes, B, tile):
    c = mc.chain_case(D, K, nodes, B)
    with _ops.option(_ops.OPT_TILE_SHAPE, tile):
        _, _, pt, lw = fused_call(c, D, K, nodes, B)
        if tile != 16:
            with _ops.option(_ops.OPT_TILE_SHAPE, 16):
                assert not torch.equal(fused_call(c, D, K, nodes, B)[2].log_q, pt.log_q), "the 16-chain kernel ran"
    assert pt.x.shape[0] == B
    moved = check_chain(f"c D={D} W={D * nodes} tile {tile}", c, pt, lw)
    if bool(moved.any()):
        # The one chain the rule lets go must be a property of that chain's DATA under this tile's arithmetic (a ReLU kink or an
        # amplified rounding on its trajectory), not of where it sits: with the batch reversed it lands in another workgroup and
        # lane, and every chain - the one that left included - must come out bit for bit.  An indexing error (a mass or noise
        # entry read for the wrong lane or row) moves with the position and fails here.
        perm = torch.arange(B).flip(0)
        cp = dict(c, eps0=c["eps0"][perm], na=c["na"][:, :, perm].contiguous(), nb=c["nb"][:, :, perm].contiguous())
        with _ops.option(_ops.OPT_TILE_SHAPE, tile):
            _, _, pt_p, lw_p = fused_call(cp, D, K, nodes, B)
        assert torch.equal(pt_p.x.cpu()[perm], pt.x.cpu()) and torch.equal(lw_p.cpu()[perm], lw.cpu())


def test_call_in_pieces_and_smc_mode_fill_the_same_mass_fields():
    """new_phase_state / enqueue_phase (fabhip_ais_phase) and SMC mode with a threshold that never resamples (fabhip_ais_run_ext)
    copy mass and max_grad from their own arguments: bit-identical to the fused call, tuning on."""
    D, K, nodes, B = mc.CHAIN_SHAPES[0]
    c = mc.chain_case(D, K, nodes, B)
    hmc, ais, pt, lw = fused_call(c, D, K, nodes, B, tune=True)
    assert not torch.equal(hmc.epsilons.cpu()[:, :1], c["eps"][:, :1].expand(M, 1))
    # in pieces
    hmc2, ais2 = chain_samplers(c, D, K, nodes, B, tune=True)
    st = ais2.new_phase_state(B, c["eps0"].to(DEV), c["na"].to(DEV), c["nb"].to(DEV))
    ais2.enqueue_phase(st, 3, 1, M)
    assert int(st["n_valid"][1]) == B
    for a, b in ((st["x"], pt.x), (st["lq"], pt.log_q), (st["lp"], pt.log_p), (st["gq"], pt.grad_log_q), (st["log_w"], lw),
                 (hmc2.epsilons, hmc.epsilons), (hmc2.common_epsilon, hmc.common_epsilon)):
        assert torch.equal(a, b)
    # SMC mode, threshold 0: the decision runs before every transition and never resamples
    hmc3, ais3 = chain_samplers(c, D, K, nodes, B, tune=True, tau=0.0)
    pt3, lw3 = ais3.sample_and_log_weights(B, eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV),
                                           noise_r=torch.full((M,), 0.37, dtype=torch.float64, device=DEV))
    assert int(ais3.last_smc[0].sum()) == 0
    for a, b in ((pt3.x, pt.x), (pt3.log_q, pt.log_q), (pt3.grad_log_q, pt.grad_log_q), (lw3, lw), (hmc3.epsilons, hmc.epsilons),
                 (hmc3.common_epsilon, hmc.common_epsilon)):
        assert torch.equal(a, b)


def test_one_rank_sharded_op_fills_the_same_mass_fields():
    """fabhip::ais_sharded_tuned on a one-rank gloo group: refuses n_outer = 2 by name (the exact sharded rule is defined for
    n_outer == 1), and with n_outer = 1 is bit-identical to the fused call with the same mass and max_grad."""
    import datetime
    import torch.distributed as dist
    D, K, nodes, B = mc.CHAIN_SHAPES[0]
    c = mc.chain_case(D, K, nodes, B)
    _, ais_two = chain_samplers(c, D, K, nodes, B, tune=True)
    with pytest.raises(_ops.FabhipError, match="n_outer == 1"):
        parallel.HipShardBackend(ais_two)._state(B)
    eps0, na, nb = c["eps0"].to(DEV), c["na"][:, :1].contiguous().to(DEV), c["nb"][:, :1].contiguous().to(DEV)
    hmc1, ais1 = chain_samplers(c, D, K, nodes, B, tune=True, n_outer=1)
    pt, lw = ais1.sample_and_log_weights(B, eps0=eps0, noise_a=na, noise_b=nb)
    hmc2, ais2 = chain_samplers(c, D, K, nodes, B, tune=True, n_outer=1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1, timeout=datetime.timedelta(seconds=60))
    try:
        pt2, lw2, _ = parallel.HipShardBackend(ais2).run_tuned(B, None, eps0, na, nb)
    finally:
        dist.destroy_process_group()
    for a, b in ((pt2.x, pt.x), (pt2.log_q, pt.log_q), (lw2, lw), (hmc2.epsilons, hmc1.epsilons), (hmc2.common_epsilon, hmc1.common_epsilon)):
        assert torch.equal(a, b)
    # ... and that call is the mass-carrying one: the same call at unit mass ends elsewhere
    hmc3, ais3 = chain_samplers(c, D, K, nodes, B, tune=True, n_outer=1)
    hmc3.mass_vector.fill_(1.0)
    assert not torch.equal(ais3.sample_and_log_weights(B, eps0=eps0, noise_a=na, noise_b=nb)[0].x, pt.x)


# ---- (d) the prefetch of repeated calls -----------------------------------------------------------------------------------------
def test_mass_changed_in_place_drops_the_prefetched_chain_initialisation():
    """Two identical calls (the second enqueues the third's chain initialisation), then `mass_vector.mul_`: the prefetch key
    changes, the piece is discarded with the generator rewound over its draw, and the third call is the first call of a fresh
    sampler built with that mass, from the generator state the second call left."""
    D, K, nodes, B = mc.CHAIN_SHAPES[0]
    c = mc.chain_case(D, K, nodes, B)
    n = 256

    def sampler(prefetch):
        hmc, ais = chain_samplers(c, D, K, nodes, B)          # step sizes frozen: a fresh sampler has the state of a used one
        ais.prefetch = prefetch
        return hmc, ais
    hmc_a, ais_a = sampler(True)
    torch.manual_seed(11)
    first = ais_a.sample_and_log_weights(n)
    ais_a.sample_and_log_weights(n)
    assert "_pf_state" in ais_a.__dict__
    old_key = ais_a.__dict__["_pf_state"][0]
    hmc_a.mass_vector.mul_(1.3)
    assert ais_a._pf_key(*ais_a._native_parts(), hmc_a, n) != old_key      # the key holds the mass vector's version
    pa, lwa = ais_a.sample_and_log_weights(n)
    # the piece made for the old key was discarded and nothing was enqueued in its place: had it been taken (a key without the
    # mass), this call would have run in pieces and left the NEXT call's chain initialisation here
    assert "_pf_state" not in ais_a.__dict__
    ais_a.sample_and_log_weights(n)
    assert ais_a.__dict__["_pf_state"][0] != old_key                        # repeated under the new key: prefetching again
    hmc_b, ais_b = sampler(False)
    torch.manual_seed(11)
    ais_b.sample_and_log_weights(n)
    ais_b.sample_and_log_weights(n)
    hmc_c, ais_c = sampler(False)
    hmc_c.mass_vector.mul_(1.3)
    assert torch.equal(hmc_c.mass_vector, hmc_a.mass_vector)
    pc, lwc = ais_c.sample_and_log_weights(n)
    assert torch.equal(pa.x, pc.x) and torch.equal(pa.log_q, pc.log_q) and torch.equal(lwa, lwc)
    assert not torch.equal(pa.x, first[0].x)


# ---- (e) the generic path, (f) the spline flow -----------------------------------------------------------------------------------
def test_generic_path_with_plugin_densities():
    """k_gen_hmc_begin / k_gen_leap_pre / k_gen_leap_post / k_gen_hmc_accept: plug-in densities evaluated by torch, D = 20."""
    D, K, nodes, B = mc.EXTRA_SHAPES[0]
    c = mc.case(D, K, nodes, B, "vector")
    base, target = mc.PlugGaussian(D), c["tgt"].to(device=DEV, dtype=torch.float32)
    hmc = make_hmc(c, base.log_prob, target.log_prob, c["mass"])
    assert not hmc.is_native
    out, lw = run_transition(c, hmc)
    check("e generic path D=20", c, out, lw)


def spline_hip(c):
    """the HIP twin of the spline case's oracle flow"""
    a = mc.SPLINE_ARGS
    hf = fa.CircularCoupledRQSFlow(c["mass"].shape[0], a["L"], a["hidden"], a["circ"], c["tail_bound"], seed=a["seed"])
    res = hf._nf_model.load_state_dict(c["nf"].state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return hf.to(DEV).requires_grad_(False)


def test_spline_flow_host_fused_and_stepwise(monkeypatch):
    """The 60-D spline set-up of test_gpu_spline.py: lanes hold the coordinates c, c + 16, c + 32, c + 48 with four different
    masses.  The host-fused op (spline_r8.h's folded leapfrog) and the step-by-step path against the oracle (x, log_q, log_p,
    log_w, as that file compares) and against each other, bit for bit."""
    D, K, nodes, B = mc.EXTRA_SHAPES[1]
    c = mc.case(D, K, nodes, B, "vector")
    hf = spline_hip(c)
    target = fa.ManyWellEnergy(D)
    outs = {}
    for mode in ("fused", "stepwise"):
        if mode == "stepwise":
            monkeypatch.setattr(fa.HamiltonianMonteCarlo, "force_stepwise", True)
        hmc = make_hmc(c, hf.log_prob, target.log_prob, c["mass"])
        assert not hmc.is_native and (hmc._spline_parts() is None) == (mode == "stepwise")
        outs[mode] = run_transition(c, hmc)
    for k in ("x", "log_q", "log_p", "grad_log_q", "grad_log_p"):
        u, v = getattr(outs["fused"][0], k), getattr(outs["stepwise"][0], k)
        assert torch.equal(u.nan_to_num(nan=7.0), v.nan_to_num(nan=7.0)), k          # (a rejected special row keeps its NaN)
    assert torch.equal(outs["fused"][1], outs["stepwise"][1])
    check("f spline D=60 host-fused", c, *outs["fused"], grad=False, may_leave=2)


# ---- (g) the defensive mixture --------------------------------------------------------------------------------------------------
def test_defensive_mixture_call_carries_the_mass():
    """k_hmc_step_mix (the MIX instantiation of the 16-chain body) through fabhip::ais_run_ext, against defensive_spec's call with
    an oracle HMC that carries the mass and max_grad."""
    D, K, nodes, B = mc.MIX_SHAPE
    c = mc.chain_case(D, K, nodes, B, mix=True)
    hmc, ais = chain_samplers(c, D, K, nodes, B, mix=True)
    assert ais.is_native and not hmc.is_native
    pt, lw = ais.sample_and_log_weights(B, eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV), sel=c["sel"].to(DEV))
    assert pt.x.shape[0] == B
    check_chain("g defensive mixture", c, pt, lw)


# ---- (h) host checks ------------------------------------------------------------------------------------------------------------
def test_a_wrong_mass_vector_is_refused_by_the_host():
    D, K, nodes, B = mc.SHAPES[0]
    c = mc.case(D, K, nodes, B, "vector")
    hf, target = hip_flow(D, K, nodes, B), fa.ManyWellEnergy(D)
    with pytest.raises(AssertionError):                                      # the reference's own check (hmc.py:32-33)
        fa.HamiltonianMonteCarlo(1, D, hf.log_prob, target.log_prob, alpha=2.0, mass_init=torch.ones(D + 1))
    for bad in _bad_masses(D):
        hmc = make_hmc(c, hf.log_prob, target.log_prob, c["mass"])
        hmc.mass_vector = bad
        pt = device_point(c["plain"])
        with pytest.raises(RuntimeError, match="fabhip: mass"):
            hmc.transition(pt, 1, mc.BETA, noise_p=c["noise_p"].to(DEV), noise_e=c["noise_e"].to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(pt.x.cpu(), c["plain"].x.float())                  # nothing ran


def _bad_masses(D):
    return (torch.ones(D + 1, device=DEV), torch.ones(D - 1, device=DEV), torch.ones(D, device=DEV, dtype=torch.float64), torch.ones(D))


def test_a_wrong_mass_vector_is_refused_on_the_fused_call_and_the_generic_and_spline_routes():
    """each route checks `mass` where it fills its own argument struct (fabhip::ais_run, hmc_generic_begin, spline_hmc_transition)"""
    D, K, nodes, B = mc.CHAIN_SHAPES[0]
    c = mc.chain_case(D, K, nodes, B)
    for bad in _bad_masses(D):
        hmc, ais = chain_samplers(c, D, K, nodes, B)
        hmc.mass_vector = bad
        with pytest.raises(RuntimeError, match="fabhip: mass"):
            ais.sample_and_log_weights(B, eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV))
    for shape, flow_of in ((mc.EXTRA_SHAPES[0], None), (mc.EXTRA_SHAPES[1], spline_hip)):
        D, K, nodes, B = shape
        c = mc.case(D, K, nodes, B, "vector")
        if flow_of is None:
            log_q, log_p = mc.PlugGaussian(D).log_prob, c["tgt"].to(device=DEV, dtype=torch.float32).log_prob
        else:
            log_q, log_p = flow_of(c).log_prob, fa.ManyWellEnergy(D).log_prob
        for bad in _bad_masses(D):
            hmc = make_hmc(c, log_q, log_p, c["mass"])
            hmc.mass_vector = bad
            pt = device_point(c["plain"])
            with pytest.raises(RuntimeError, match="fabhip: mass"):
                hmc.transition(pt, 1, mc.BETA, noise_p=c["noise_p"].to(DEV), noise_e=c["noise_e"].to(DEV))
            torch.cuda.synchronize()
            assert torch.equal(pt.x.cpu(), c["plain"].x.float())


def test_load_state_dict_with_another_mass_vector_is_picked_up_by_the_next_transition():
    D, K, nodes, B = mc.SHAPES[2]
    c = mc.case(D, K, nodes, B, "vector")
    hf, target = hip_flow(D, K, nodes, B), fa.ManyWellEnergy(D)
    hmc = make_hmc(c, hf.log_prob, target.log_prob, mc.SCALAR_MASS)
    ref, lw_ref = run_transition(c, make_hmc(c, hf.log_prob, target.log_prob, c["mass"]))
    before, _ = run_transition(c, hmc)
    sd = copy.deepcopy(hmc.state_dict())
    sd["mass_vector"] = c["mass"].clone()
    hmc.load_state_dict(sd)
    after, lw = run_transition(c, hmc)
    assert torch.equal(after.x, ref.x) and torch.equal(after.log_q, ref.log_q) and torch.equal(lw, lw_ref)
    assert not torch.equal(before.x, after.x)
