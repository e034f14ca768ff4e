"""Flow-proposal independence moves on the GPU (n_flow_moves; include/fabhip.h: fabhip_flow_move, fabhip_flow_moves_args) against
their specification (tests/flow_move_spec.py).

1  fabhip::flow_move against the spec, bit for bit: the proposal's Point comes from the op's own three steps run through public
   calls (flow.sample_and_log_prob, create_point); its float32 densities go into the spec.
2  the fused call equals its step-by-step composition (phase op per transition, fabhip::flow_move in between), bit for bit.
3  n_flow_moves = 0 is the call without the argument; with moves on the draws come after noise_a / noise_b, g before h.
4  a beta = 0 step accepts every live row.
5  composition: SMC mode, adaptive schedules, fast mode, HIP-graph replay, determinism.
6  refusals and validation, Python and C ABI.
7  FABModel / PrioritisedBufferTrainer.

Shapes: (D, K, nodes) = (32, 3, 10) - hidden width 320 - and (6, 3, 5) - width 30 - as in tests/test_gpu_ais_routes.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import adaptive_spec
import flow_move_spec as spec
import smc_spec

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _lib, _ops, parallel            # noqa: E402
from fab_torch_amd.ais import operator_slots                     # noqa: E402
from fab_torch_amd.transition_operators import create_point      # noqa: E402

DEV = "cuda"
M, L = 4, 3
WIDE, NARROW = (32, 3, 10), (6, 3, 5)
F32 = dict(dtype=torch.float32, device=DEV)


def _flow(shape, seed=0):
    D, K, nodes = shape
    torch.manual_seed(seed)
    flow = fa.make_wrapped_normflow_realnvp(D, K, nodes, act_norm=False).to(DEV).requires_grad_(False)
    with torch.no_grad():
        for l1, l2, l3, aff in flow._layers():
            l3.weight.add_(0.01 * torch.randn_like(l3.weight))
    return flow


def _sampler(shape, hmc=True, p_target=False, eval_mode=False, m=M, epsilon=0.1, target=None, **kw):
    D = shape[0]
    flow = _flow(shape)
    target = fa.ManyWellEnergy(D) if target is None else target
    alpha = None if p_target else 2.0
    if hmc:
        op = fa.HamiltonianMonteCarlo(m, D, flow.log_prob, target.log_prob, alpha=alpha, p_target=p_target, epsilon=epsilon, L=L,
                                      eval_mode=eval_mode).to(DEV)
    else:
        op = fa.Metropolis(m, D, flow.log_prob, target.log_prob, n_updates=2, alpha=alpha, p_target=p_target, max_step_size=0.4,
                           min_step_size=0.1, adjust_step_size=True, eval_mode=eval_mode).to(DEV)
    return flow, target, op, fa.AnnealedImportanceSampler(flow, target.log_prob, op, p_target, alpha, m, **kw)


def _noise(B, D, k, hmc=True, seed=0, m=M):
    g = torch.Generator().manual_seed(300 + seed)
    n = 1 if hmc else 2
    eps0 = torch.randn(B, D, generator=g)
    na = torch.randn(m, n, B, D, generator=g)
    nb = torch.empty(m, n, B).exponential_(1.0, generator=g) if hmc else torch.rand(m, n, B, generator=g)
    ng = torch.randn(m, max(k, 1), B, D, generator=g)[:, :k].contiguous()
    nh = torch.empty(m, max(k, 1), B).exponential_(1.0, generator=g)[:, :k].contiguous()
    nr = torch.rand(m, generator=g, dtype=torch.float64)
    return tuple(t.to(DEV) for t in (eps0, na, nb, ng, nh, nr))


def _step_state(op):
    return (op.epsilons, op.common_epsilon) if isinstance(op, fa.HamiltonianMonteCarlo) else (op.noise_scalings,)


def _np_point(pt):
    c = lambda t: None if t is None else t.detach().cpu().numpy()      # noqa: E731
    return (c(pt[0]), c(pt[1]), c(pt[2]), c(pt[3]), c(pt[4]))


def _proposal(flow, target, g, hmc):
    """The op's first two steps through public calls: the proposal's Point as a tuple of device tensors."""
    x, _ = flow.sample_and_log_prob((g.shape[0],), eps=g)
    p = create_point(x, flow, target, hmc)
    return (p.x, p.log_q, p.log_p, p.grad_log_q, p.grad_log_p)


def _move_op(flow, target, cur, n_valid, beta, alpha, p_target, g, h):
    return _ops.load().flow_move(*flow.native(), *target.native_target(), cur[0], cur[1], cur[2], cur[3], cur[4], n_valid,
                                 float(beta), float(alpha), bool(p_target), g, h, _ops.precision_of(flow))


def _assert_point_equals_spec(cur, want, tag):
    for name, got, ref in zip(("x", "log_q", "log_p", "grad_log_q", "grad_log_p"), cur, want):
        if got is None:
            assert ref is None
            continue
        assert torch.equal(got.cpu(), torch.from_numpy(ref)), f"{tag}: {name} differs from the spec"


# ---- 1. the op against the spec ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
@pytest.mark.parametrize("shape", [NARROW, WIDE])
def test_flow_move_equals_the_spec_bit_for_bit(shape, hmc):
    D = shape[0]
    flow, target = _flow(shape), fa.ManyWellEnergy(D)
    ops = _ops.load()
    gen = torch.Generator().manual_seed(5)
    n_acc_seen = set()
    for B in (5, 37, 200):
        g0, g = torch.randn(B, D, generator=gen).to(DEV), torch.randn(B, D, generator=gen).to(DEV)
        h = torch.empty(B).exponential_(1.0, generator=gen).to(DEV)
        prop = _proposal(flow, target, g, hmc)
        start = _proposal(flow, target, g0, hmc)
        for n_valid in (B, B - 3, 0):
            nv = torch.tensor([n_valid], dtype=torch.int32, device=DEV)
            for beta in (0.0, 0.3, 1.0):
                for p_target, alpha in ((True, 0.0), (False, 2.0)):
                    c_q, c_p = spec.anneal_coefs(beta, alpha, p_target)
                    dev_c = ops.anneal_coefs(beta, alpha, p_target)
                    assert (float(c_q), float(c_p)) == (dev_c[0], dev_c[1])
                    cur = tuple(None if t is None else t.clone() for t in start)
                    want = spec.move(_np_point(start), _np_point(prop), h.cpu().numpy(), c_q, c_p, n_valid)
                    frac, count = _move_op(flow, target, cur, nv if n_valid != B else None, beta, alpha, p_target, g, h)
                    tag = f"B={B} n_valid={n_valid} beta={beta} p_target={p_target}"
                    moved = (cur[1] != start[1]) | (cur[2] != start[2]) | (cur[0] != start[0]).any(1)
                    assert torch.equal(moved.cpu(), torch.from_numpy(want.accept)), f"{tag}: accept mask"
                    _assert_point_equals_spec(cur, want.point, tag)
                    assert count.dtype == torch.int32 and int(count) == want.n_accept, tag
                    assert frac.dtype == torch.float32 and torch.equal(frac.cpu(), torch.tensor([want.p_accept])), tag
                    if beta == 0.0:
                        assert want.n_accept == n_valid
                    n_acc_seen.add(0 < want.n_accept < n_valid)
    assert n_acc_seen == {True, False}                      # partial acceptance occurred, and so did all-or-none


@pytest.mark.parametrize("hmc", [True, False])
def test_flow_move_rejects_proposals_with_non_finite_density(hmc):
    D, B = NARROW[0], 37
    flow, target = _flow(NARROW), fa.ManyWellEnergy(D)
    gen = torch.Generator().manual_seed(6)
    g0, g = torch.randn(B, D, generator=gen), torch.randn(B, D, generator=gen)
    g[3, 0], g[20, 1], g[36, 5] = float("nan"), float("inf"), float("-inf")
    g0, g = g0.to(DEV), g.to(DEV)
    h = torch.full((B,), 1e30, **F32)                       # (a finite row accepts whatever its delta is)
    prop, start = _proposal(flow, target, g, hmc), _proposal(flow, target, g0, hmc)
    bad = ~(torch.isfinite(prop[1]) & torch.isfinite(prop[2]))
    assert bad[3] and bad[20] and bad[36] and int(bad.sum()) == 3
    c_q, c_p = spec.anneal_coefs(0.3, 2.0, False)
    cur = tuple(None if t is None else t.clone() for t in start)
    want = spec.move(_np_point(start), _np_point(prop), h.cpu().numpy(), c_q, c_p)
    frac, count = _move_op(flow, target, cur, None, 0.3, 2.0, False, g, h)
    assert want.n_accept == B - 3 == int(count) and not want.accept[[3, 20, 36]].any()
    _assert_point_equals_spec(cur, want.point, "non-finite proposals")
    assert all(torch.isfinite(t).all() for t in cur if t is not None)
    assert torch.equal(frac.cpu(), torch.tensor([want.p_accept]))


# ---- 2. fused call == step-by-step composition -------------------------------------------------------------------------------------
def _composed(ais, op, B, eps0, na, nb, ng, nh, k, stop_after_moves_of=None):
    """The call assembled from new_phase_state / enqueue_phase per transition with fabhip::flow_move in between (`ais` has
    n_flow_moves = 0: its pieces are the plain phase op's)."""
    flow, target = ais._native_parts()
    st = ais.new_phase_state(B, eps0, na, nb)
    ais.enqueue_phase(st, 1, 1, 0)
    fracs = []
    for j in range(1, ais.n_intermediate_distributions + 1):
        for m in range(k):
            cur = (st["x"], st["lq"], st["lp"], st["gq"], st["gp"])
            fracs.append(_move_op(flow, target, cur, st["n_valid"], float(ais.B_space[j]), ais._alpha_arg, ais.p_target,
                                  ng[j - 1, m], nh[j - 1, m])[0])
        if stop_after_moves_of == j:
            return st, fracs
        ais.enqueue_phase(st, 0, j, j)
    ais.enqueue_phase(st, 2, 1, 0)
    return st, torch.cat(fracs).view(-1, k)


ROUTES = {"4-chain": (WIDE, 200, True, 0), "8-chain": (WIDE, 1200, True, 0), "16-chain": (NARROW, 200, True, 16),
          "metropolis": (WIDE, 200, False, 0)}


def _fused_vs_composed(shape, B, hmc, tile, k, fast=False):
    D = shape[0]
    eps0, na, nb, ng, nh, _ = _noise(B, D, k, hmc)
    with _ops.option(_ops.OPT_TILE_SHAPE, tile), fa.fast_mode(fast):
        _, _, op1, ais1 = _sampler(shape, hmc, n_flow_moves=k)
        pt, log_w, n_valid, stats, _, _ = ais1.run(B, eps0, na, nb, noise_g=ng, noise_h=nh)
        _, _, op2, ais2 = _sampler(shape, hmc)
        st, fracs = _composed(ais2, op2, B, eps0, na, nb, ng, nh, k)
    n1 = int(n_valid[1])
    assert n1 == int(st["n_valid"][1]) and 0 < n1 <= B and torch.equal(n_valid, st["n_valid"])
    for name, u, v in (("x", pt.x, st["x"]), ("log_q", pt.log_q, st["lq"]), ("log_p", pt.log_p, st["lp"]), ("log_w", log_w, st["log_w"])):
        assert torch.equal(u[:n1], v[:n1]), f"{name} differs between the fused call and its composition"
    assert torch.equal(stats[:6], st["stats"][:6])
    for u, v in zip(_step_state(op1), _step_state(op2)):
        assert torch.equal(u, v), "step sizes differ"
    assert ais1.last_flow_moves.shape == (M, k) and torch.equal(ais1.last_flow_moves, fracs)
    fm = ais1.last_flow_moves
    assert bool(((fm >= 0) & (fm < 1)).all()) and bool((fm[0] > 0).all())      # (moves happened: the comparison is not vacuous)
    return ais1, op1


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_fused_call_equals_its_step_by_step_composition(route, k):
    shape, B, hmc, tile = ROUTES[route]
    _, op = _fused_vs_composed(shape, B, hmc, tile, k)
    start = _sampler(shape, hmc)[2]
    assert not torch.equal(_step_state(op)[0], _step_state(start)[0])      # tuning is on: the step sizes moved


# ---- 3. moves off is today's call; the order of the draws ---------------------------------------------------------------------------
def _rng():
    return torch.cuda.get_rng_state(torch.cuda.current_device())


@pytest.mark.parametrize("hmc", [True, False])
def test_zero_moves_is_the_call_without_the_argument(hmc):
    B, outs = 200, []
    for kw in ({}, {"n_flow_moves": 0}):
        _, _, op, ais = _sampler(WIDE, hmc, **kw)
        torch.manual_seed(11)
        res = []
        for _ in range(2):
            pt, lw = ais.sample_and_log_weights(B)
            res += [pt.x.clone(), pt.log_q.clone(), pt.log_p.clone(), lw.clone()]
        outs.append(res + [t.clone() for t in _step_state(op)] + [_rng()])
        assert ais.last_flow_moves is None and "flow_move_p_accept_dist0" not in ais.get_logging_info()
    assert len(outs[0]) == len(outs[1]) and all(torch.equal(u, v) for u, v in zip(*outs))


@pytest.mark.parametrize("tau", [None, 2.0])
def test_absent_draws_come_after_the_transition_noise_g_before_h(tau):
    D, B, k = WIDE[0], 200, 2
    _, _, op1, ais1 = _sampler(WIDE, n_flow_moves=k, resample_threshold=tau)
    torch.manual_seed(12)
    pt1, lw1 = ais1.sample_and_log_weights(B)
    rng1 = _rng()
    _, _, op2, ais2 = _sampler(WIDE, n_flow_moves=k, resample_threshold=tau)
    torch.manual_seed(12)
    eps0 = torch.randn((B, D), **F32)
    na = torch.randn((M, 1, B, D), **F32)
    nb = torch.empty((M, 1, B), **F32).exponential_(1.0)
    ng = torch.randn((M, k, B, D), **F32)
    nh = torch.empty((M, k, B), **F32).exponential_(1.0)
    nr = torch.rand(M, dtype=torch.float64, device=DEV) if tau is not None else None
    pt2, lw2 = ais2.sample_and_log_weights(B, eps0=eps0, noise_a=na, noise_b=nb, noise_r=nr, noise_g=ng, noise_h=nh)
    assert torch.equal(rng1, _rng())
    assert torch.equal(pt1.x, pt2.x) and torch.equal(lw1, lw2) and torch.equal(ais1.last_flow_moves, ais2.last_flow_moves)
    assert all(torch.equal(u, v) for u, v in zip(_step_state(op1), _step_state(op2)))
    info = ais1.get_logging_info()
    fm = ais1.last_flow_moves.cpu()
    assert info["flow_move_p_accept_dist0"] == pytest.approx(float(fm[0].mean()), abs=1e-7)
    assert info[f"flow_move_p_accept_dist{M - 1}"] == pytest.approx(float(fm[M - 1].mean()), abs=1e-7)


# ---- 4. a step at beta = 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_every_live_row_is_accepted_at_beta_zero(hmc):
    shape, B, k, m = NARROW, 200, 2, 2
    D = shape[0]
    sched = [0.0, 0.0, 0.5, 1.0]
    eps0, na, nb, ng, nh, _ = _noise(B, D, k, hmc, seed=4, m=m)
    eps0[7] = float("inf")                                   # a chain the "chain init" filter removes
    flow, target, op, ais = _sampler(shape, hmc, m=m, n_flow_moves=k, distribution_spacing_type=sched)
    pt, log_w, n_valid, _, _, _ = ais.run(B, eps0, na, nb, noise_g=ng, noise_h=nh)
    fm = ais.last_flow_moves.cpu()
    assert int(n_valid[0]) == B - 1
    assert torch.equal(fm[0], torch.ones(k)), f"acceptance at beta = 0: {fm[0].tolist()}"
    assert bool((fm[1] < 1).all())
    # the same call stopped behind the moves of step 1 through the phase op: the live rows ARE the last proposals
    _, _, op2, ais2 = _sampler(shape, hmc, m=m, distribution_spacing_type=sched)
    st, fracs = _composed(ais2, op2, B, eps0, na, nb, ng, nh, k, stop_after_moves_of=1)
    n0 = int(st["n_valid"][0])
    assert n0 == B - 1 and all(float(f) == 1.0 for f in fracs)
    prop = _proposal(flow, target, ng[0, k - 1], hmc)
    for name, got, ref in zip(("x", "log_q", "log_p", "grad_log_q", "grad_log_p"), (st["x"], st["lq"], st["lp"], st["gq"], st["gp"]),
                              prop):
        if ref is not None:
            assert torch.equal(got[:n0], ref[:n0]), f"{name} of the live rows is not the last proposal's"


# ---- 5. composition ------------------------------------------------------------------------------------------------------------------
def _phase_args(ais, op, st, phases, j0, j1):
    flow, target = ais._native_parts()
    kind, s = operator_slots(op)
    return (*ais._call_head(flow, target, kind), int(phases), int(j0), int(j1), st["eps0"], st["noise_a"], st["noise_b"], *s[:8],
            st["x"], st["lq"], st["lp"], st["gq"], st["gp"], st["log_w"], st["n_valid"], st["stats"], None, *s[8:], None, None,
            _ops.precision_of(flow))


@pytest.mark.parametrize("hmc", [True, False])
def test_smc_mode_with_moves_follows_both_specs(hmc):
    """resample_threshold = 2 resamples before every transition.  Teacher-forced: the device's own log_w_pre goes into the SMC
    spec (ancestors EQUAL), the device's own point behind the resampling step into the move spec (point EQUAL), and the fused
    call equals the stepped one."""
    shape, B, k, tau = WIDE, 200, 1, 2.0
    D = shape[0]
    eps0, na, nb, ng, nh, nr = _noise(B, D, k, hmc, seed=7)
    flow, target, op1, ais1 = _sampler(shape, hmc, n_flow_moves=k, resample_threshold=tau)
    pt, log_w, n_valid, stats, _, _ = ais1.run(B, eps0, na, nb, noise_r=nr, trace=True, noise_g=ng, noise_h=nh)
    resampled, ess, anc, lw_pre = ais1.last_smc
    n0 = int(n_valid[0])
    assert n0 == B and bool((resampled == 1).all())
    for j in range(M):
        d = smc_spec.decide(lw_pre[j, :n0].cpu().numpy(), tau, float(nr[j]))
        assert d.resampled and np.array_equal(anc[j, :n0].cpu().numpy().astype(np.int64), d.ancestors), f"step {j + 1}: ancestors"
    # stepped: resampling step alone, the move against the spec, the transition alone
    ops = _ops.load()
    _, _, op2, ais2 = _sampler(shape, hmc)
    st = ais2.new_phase_state(B, eps0, na, nb)
    ais2.enqueue_phase(st, 1, 1, 0)
    rec = (torch.zeros(M, dtype=torch.int32, device=DEV), torch.zeros(M, **F32), torch.zeros((M, B), dtype=torch.int32, device=DEV),
           torch.zeros((M, B), **F32))
    fracs = []
    for j in range(1, M + 1):
        ops.ais_phase_smc(*_phase_args(ais2, op2, st, 0, j, j), tau, nr, True, *rec, 0)
        cur = (st["x"], st["lq"], st["lp"], st["gq"], st["gp"])
        before = _np_point(cur)
        beta = float(ais2.B_space[j])
        want = spec.move(before, _np_point(_proposal(flow, target, ng[j - 1, 0], hmc)), nh[j - 1, 0].cpu().numpy(),
                         *spec.anneal_coefs(beta, 2.0, False), n0)
        fracs.append(_move_op(flow, target, cur, st["n_valid"], beta, 2.0, False, ng[j - 1, 0], nh[j - 1, 0])[0])
        _assert_point_equals_spec(cur, want.point, f"step {j}")
        assert float(fracs[-1]) == float(want.p_accept) and want.n_accept < n0 and (j > 1 or want.n_accept > 0)
        ais2.enqueue_phase(st, 0, j, j)
    ais2.enqueue_phase(st, 2, 1, 0)
    assert torch.equal(rec[2], anc) and torch.equal(rec[3], lw_pre)
    assert torch.equal(pt.x, st["x"]) and torch.equal(log_w, st["log_w"]) and torch.equal(pt.log_q, st["lq"])
    assert torch.equal(ais1.last_flow_moves, torch.cat(fracs).view(M, k))
    assert all(torch.equal(u, v) for u, v in zip(_step_state(op1), _step_state(op2)))


@pytest.mark.parametrize("tau", [None, 0.5])
def test_adaptive_schedule_with_moves_follows_the_adaptive_spec(tau):
    shape, B, k, rho = NARROW, 100, 1, 0.7
    D = shape[0]
    eps0, na, nb, ng, nh, nr = _noise(B, D, k, seed=8)
    _, _, op, ais = _sampler(shape, eval_mode=True, epsilon=0.05, n_flow_moves=k, distribution_spacing_type="adaptive",
                             ess_decay=rho, resample_threshold=tau)
    pt, log_w, n_valid, _, _, _ = ais.run(B, eps0, na, nb, trace=True, noise_r=nr if tau is not None else None, noise_g=ng,
                                          noise_h=nh)
    n0 = int(n_valid[0])
    betas = ais.last_betas
    assert n0 == B and betas.shape == (M + 2,) and float(betas[0]) == 0.0 and float(betas[-1]) == 1.0
    assert bool((betas[1:] >= betas[:-1]).all())
    assert 1 <= len(ais.last_adaptive) <= M
    for d in ais.last_adaptive:
        lw, lq, lp = (t[:n0].cpu().numpy() for t in d.inputs)
        want = adaptive_spec.next_beta(lw, lq, lp, d.beta, 2.0, False, rho)
        assert d.beta_next == want.beta_next and float(betas[d.step + 1]) == want.beta_next, f"decision {d.step}"
        assert d.ess0 == want.as_out4()[1]
    fm = ais.last_flow_moves
    assert fm.shape == (M, k) and bool(((fm >= 0) & (fm <= 1)).all()) and torch.isfinite(log_w[:int(n_valid[1])]).all()
    # the same schedule as the caller's own through the fused call: the stepped driver's moves are the fused call's
    _, _, op2, ais2 = _sampler(shape, eval_mode=True, epsilon=0.05, n_flow_moves=k, distribution_spacing_type=betas.tolist(),
                               resample_threshold=tau)
    pt2, log_w2, _, _, _, _ = ais2.run(B, eps0, na, nb, noise_r=nr if tau is not None else None, noise_g=ng, noise_h=nh)
    assert torch.equal(pt.x, pt2.x) and torch.equal(fm, ais2.last_flow_moves)


def test_fast_mode_call_equals_its_own_composition():
    _fused_vs_composed(WIDE, 200, True, 0, 1, fast=True)


def test_two_identical_calls_are_bit_identical():
    B, k = 1200, 2
    eps0, na, nb, ng, nh, _ = _noise(B, WIDE[0], k, seed=9)
    runs = []
    for _ in range(2):
        _, _, op, ais = _sampler(WIDE, n_flow_moves=k)
        pt, log_w, n_valid, stats, _, _ = ais.run(B, eps0, na, nb, noise_g=ng, noise_h=nh)
        runs.append((pt.x, pt.log_q, pt.log_p, log_w, n_valid, stats[:6], ais.last_flow_moves, *[t.clone() for t in _step_state(op)]))
    assert all(torch.equal(u, v) for u, v in zip(*runs))


def test_call_with_moves_replays_from_a_hip_graph():
    """One captured call (a single stream, no parallel branches) replays on two sets of inputs and gives what the eager call
    gives on each: no launch depends on a decision, the accept kernel's count word is zero again after every launch."""
    B, k = 256, 2
    D = WIDE[0]
    _, _, op, ais = _sampler(WIDE, eval_mode=True, n_flow_moves=k)
    in0, in1 = _noise(B, D, k, seed=10)[:5], _noise(B, D, k, seed=11)[:5]
    static = [t.clone() for t in in0]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            ais.run(B, static[0], static[1], static[2], noise_g=static[3], noise_h=static[4])
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pt, log_w, n_valid, stats, _, _ = ais.run(B, static[0], static[1], static[2], noise_g=static[3], noise_h=static[4])
        fm = ais.last_flow_moves
    for inp in (in0, in1, in0):
        for dst, src in zip(static, inp):
            dst.copy_(src)
        g.replay(); torch.cuda.synchronize()
        got = (pt.x.clone(), log_w.clone(), fm.clone())
        pe, lwe, _, _, _, _ = ais.run(B, inp[0], inp[1], inp[2], noise_g=inp[3], noise_h=inp[4])
        assert all(torch.equal(u, v) for u, v in zip(got, (pe.x, lwe, ais.last_flow_moves)))
        assert bool((fm[0] > 0).all())


# ---- 6. refusals and validation ----------------------------------------------------------------------------------------------------
def test_refused_routes_name_themselves():
    from torch_dist_plugin import WrappedTorchDist
    D, B = NARROW[0], 64
    target = fa.ManyWellEnergy(D)
    with pytest.raises(_ops.FabhipError, match="n_flow_moves"):
        _sampler(NARROW, n_flow_moves=-1)
    for bad in (1.5, True, "2"):
        with pytest.raises(_ops.FabhipError, match="n_flow_moves"):
            _sampler(NARROW, n_flow_moves=bad)
    # the generic path
    base = WrappedTorchDist(torch.distributions.MultivariateNormal(torch.zeros(D, device=DEV), scale_tril=torch.eye(D, device=DEV)))
    hmc = fa.HamiltonianMonteCarlo(M, D, base.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.2, L=L).to(DEV)
    ais = fa.AnnealedImportanceSampler(base, target.log_prob, hmc, False, 2.0, M, n_flow_moves=1)
    with pytest.raises(_ops.FabhipError, match="generic path"):
        ais.sample_and_log_weights(B)
    # a defensive mixture
    flow = _flow(NARROW)
    mix = fa.DefensiveMixtureDistribution(flow).to(DEV)
    hmc = fa.HamiltonianMonteCarlo(M, D, mix.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.2, L=L).to(DEV)
    ais = fa.AnnealedImportanceSampler(mix, target.log_prob, hmc, False, 2.0, M, n_flow_moves=1)
    for call in (ais.sample_and_log_weights, ais.run):
        with pytest.raises(_ops.FabhipError, match="DefensiveMixtureDistribution"):
            call(B)
    # the fused spline call
    tb = torch.full((D,), 5.0); tb[0] = float(np.pi)
    sflow = fa.CircularCoupledRQSFlow(D, 2, 16, (0,), tb).to(DEV)
    hmc = fa.HamiltonianMonteCarlo(M, D, sflow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.2, L=L).to(DEV)
    ais = fa.AnnealedImportanceSampler(sflow, target.log_prob, hmc, False, 2.0, M, n_flow_moves=1)
    assert ais._spline_parts() is not None
    with pytest.raises(_ops.FabhipError, match="spline"):
        ais.sample_and_log_weights(B)
    # both sharded samplers
    _, _, _, ais = _sampler(NARROW, n_flow_moves=2)
    with pytest.raises(_ops.FabhipError, match="n_flow_moves=2.*sharded"):
        parallel.ShardedAnnealedImportanceSampler(ais).sample_and_log_weights(B)
    with pytest.raises(_ops.FabhipError, match="n_flow_moves=2.*sharded"):
        parallel.ShardedAIS(ais.sample_and_log_weights).sample_and_log_weights(B)
    # a sampler restored from a state that predates the setting reads 0; the setting is settable
    del ais.__dict__["_n_flow_moves"]
    assert ais.n_flow_moves == 0
    ais.n_flow_moves = 1
    assert ais.n_flow_moves == 1


def test_wrong_draws_are_refused():
    D, B, k = NARROW[0], 64, 2
    _, _, _, ais = _sampler(NARROW, n_flow_moves=k)
    g, h = torch.randn((M, k, B, D), **F32), torch.empty((M, k, B), **F32).exponential_(1.0)
    for bad_g, bad_h, what in ((g[:, :1], h, "noise_g"), (g.double(), h, "noise_g"), (g, h[..., :-1], "noise_h"),
                               (g, h.double(), "noise_h"), (g, None, "both"), (None, h, "both"), (g.cpu().numpy(), h, "noise_g")):
        with pytest.raises(_ops.FabhipError, match=what):
            ais.run(B, noise_g=bad_g, noise_h=bad_h)
    ais.n_flow_moves = 0
    with pytest.raises(_ops.FabhipError, match="n_flow_moves"):
        ais.run(B, noise_g=g, noise_h=h)
    ops = _ops.load()
    flow, target = ais._native_parts()
    x = torch.randn((B, D), **F32)
    p = create_point(x, flow, target, True)
    with pytest.raises(RuntimeError, match="noise_g"):
        ops.flow_move(*flow.native(), *target.native_target(), p.x, p.log_q, p.log_p, p.grad_log_q, p.grad_log_p, None, 0.5, 2.0,
                      False, g[0, 0, :-1], h[0, 0], 0)
    with pytest.raises(RuntimeError, match="both gradient fields"):
        ops.flow_move(*flow.native(), *target.native_target(), p.x, p.log_q, p.log_p, p.grad_log_q, None, None, 0.5, 2.0, False,
                      g[0, 0], h[0, 0], 0)


def test_c_entry_refuses_partials_a_mixture_and_null_noise():
    D, K, nodes = NARROW
    B, k = 64, 1
    flow, target, op, ais = _sampler(NARROW, n_flow_moves=k)
    lib = _lib.load()
    eps0, na, nb, ng, nh, _ = _noise(B, D, k)
    packed, _, _, W = flow.native()
    a = _lib.AisArgs()
    a.flow = _lib.Flow(D, K, W, packed.data_ptr())
    kind, prm, _, _ = target.native_target()
    a.target = _lib.Target(kind, D, prm[0], prm[1], prm[2], prm[3], 0, None, None)
    betas = (C.c_double * (M + 2))(*[float(b) for b in ais.B_space])
    a.B, a.M, a.betas, a.alpha, a.p_target, a.transition = B, M, betas, 2.0, 0, _lib.TRANSITION_HMC
    a.eps0, a.noise_a, a.noise_b = eps0.data_ptr(), na.data_ptr(), nb.data_ptr()
    eps_c, ceps_c = op.epsilons.clone(), op.common_epsilon.clone()
    a.step_state, a.common_epsilon, a.mass = eps_c.data_ptr(), ceps_c.data_ptr(), op.mass_vector.data_ptr()
    a.n_inner, a.L, a.max_grad, a.target_p_accept, a.tune = 1, L, op.max_grad, op.target_p_accept, 1
    x, lq, lp, lw = torch.empty(B, D, **F32), torch.empty(B, **F32), torch.empty(B, **F32), torch.empty(B, **F32)
    gq, gp = torch.empty(B, D, **F32), torch.empty(B, D, **F32)
    nv, st = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(16, **F32)
    a.point = _lib.Point(x.data_ptr(), lq.data_ptr(), lp.data_ptr(), gq.data_ptr(), gp.data_ptr())
    a.log_w, a.n_valid, a.stats = lw.data_ptr(), nv.data_ptr(), st.data_ptr()
    def ext(smc=None, mix=None, moves=None):                  # fabhip_ais_ext over the members given (the rest NULL)
        return C.byref(_lib.AisExt(*(None if m is None else C.pointer(m) for m in (smc, mix, moves))))

    on, k1 = _lib.SmcArgs(enabled=1), _lib.FlowMovesArgs(n_moves=1)
    nbytes = lib.fabhip_ais_ext_workspace_bytes(B, D, 1, ext(moves=k1))
    assert nbytes >= lib.fabhip_ais_workspace_bytes(B, D, 1) + B * (3 * D + 2) * 4
    assert lib.fabhip_ais_ext_workspace_bytes(B, D, 1, ext(smc=on, moves=k1)) >= \
        lib.fabhip_ais_ext_workspace_bytes(B, D, 1, ext(smc=on)) + B * (3 * D + 2) * 4
    assert lib.fabhip_flow_move_workspace_bytes(B, D) >= B * (3 * D + 2) * 4
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    a.workspace, a.workspace_bytes = (ws.data_ptr() + 255) // 256 * 256, nbytes
    fracs = torch.full((M, k), -1.0, **F32)
    mv = _lib.FlowMovesArgs(k, ng.data_ptr(), nh.data_ptr(), fracs.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    slab = torch.zeros(int(lib.fabhip_hmc_partials_floats(B)), **F32)
    EINVAL, ENOTSUP, ENOSPC = -1, -2, -4
    # sharded chains
    assert lib.fabhip_ais_phase_ext(C.byref(a), ext(moves=mv), 0, 1, 1, _lib.ptr(slab), stream) == ENOTSUP
    # a defensive mixture
    loc, ls, logit, sel = torch.zeros(D, **F32), torch.zeros(D, **F32), torch.zeros(1, **F32), torch.rand(B, **F32)
    mix = _lib.DefensiveArgs(1, loc.data_ptr(), ls.data_ptr(), logit.data_ptr(), sel.data_ptr())
    assert lib.fabhip_ais_run_ext(C.byref(a), ext(mix=mix, moves=mv), stream) == ENOTSUP
    # null noise with moves to run, a negative count, a workspace without the proposal buffers
    for g_ptr, h_ptr in ((None, nh.data_ptr()), (ng.data_ptr(), None)):
        assert lib.fabhip_ais_run_ext(C.byref(a), ext(moves=_lib.FlowMovesArgs(k, g_ptr, h_ptr, None)), stream) == EINVAL
    assert lib.fabhip_ais_run_ext(C.byref(a), ext(moves=_lib.FlowMovesArgs(-1, ng.data_ptr(), nh.data_ptr(), None)), stream) == EINVAL
    a.workspace_bytes = lib.fabhip_ais_workspace_bytes(B, D, 1)
    assert lib.fabhip_ais_run_ext(C.byref(a), ext(moves=mv), stream) == ENOSPC
    a.workspace_bytes = nbytes
    torch.cuda.synchronize()
    assert bool((fracs == -1).all())                          # nothing ran
    # and the call itself through the C ABI equals the op
    _lib.check(lib.fabhip_ais_run_ext(C.byref(a), ext(moves=mv), stream), "ais_run_ext")
    pt, log_w, n_valid, stats, _, _ = ais.run(B, eps0, na, nb, noise_g=ng, noise_h=nh)
    assert torch.equal(nv, n_valid) and torch.equal(pt.x, x) and torch.equal(log_w, lw) and torch.equal(ais.last_flow_moves, fracs)
    assert torch.equal(op.epsilons, eps_c)
    # n_moves = 0 through the same entry is the plain call
    x0, lw0 = x.clone(), lw.clone()
    eps_c.copy_(_sampler(NARROW)[2].epsilons); ceps_c.copy_(_sampler(NARROW)[2].common_epsilon)
    _lib.check(lib.fabhip_ais_run_ext(C.byref(a), ext(moves=_lib.FlowMovesArgs(0, None, None, None)), stream), "k = 0")
    x1, lw1 = x.clone(), lw.clone()
    eps_c.copy_(_sampler(NARROW)[2].epsilons); ceps_c.copy_(_sampler(NARROW)[2].common_epsilon)
    _lib.check(lib.fabhip_ais_run(C.byref(a), stream), "ais_run")
    assert torch.equal(x, x1) and torch.equal(lw, lw1) and not torch.equal(x0, x1)


# ---- 7. through the model and the trainer -----------------------------------------------------------------------------------------
def test_trainer_runs_with_moves_on():
    Dt, Mt, B = 6, 4, 256
    torch.manual_seed(1)
    flow = fa.make_wrapped_normflow_realnvp(Dt, 4, 10, act_norm=False).to(DEV)
    target = fa.ManyWellEnergy(Dt)
    hmc = fa.HamiltonianMonteCarlo(Mt, Dt, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.2, L=5).to(DEV)
    model = fa.FABModel(flow, target, Mt, alpha=2.0, transition_operator=hmc, loss_type="fab_alpha_div", ais_n_flow_moves=1)
    ais = model.annealed_importance_sampler
    assert ais.n_flow_moves == 1

    def initial_sampler():
        pt, lw = ais.sample_and_log_weights(B, logging=False)
        return pt.x, lw, pt.log_q
    buf = fa.PrioritisedReplayBuffer(Dt, 8 * B, 2 * B, initial_sampler, device=DEV)
    opt = fa.FlatAdam(flow, lr=1e-4)
    trainer = fa.PrioritisedBufferTrainer(model, opt, buf, alpha=2.0, n_batches_buffer_sampling=2)
    for i in range(2):
        info = trainer.step(i, B)
        assert np.isfinite(info["loss"]), (i, info)
        for key in ("flow_move_p_accept_dist0", f"flow_move_p_accept_dist{Mt - 1}"):
            assert 0.0 <= info[key] <= 1.0, (key, info[key])
        assert 0 < info["ess_ais"] <= 1 and np.isfinite(info["log_Z"])
    assert ais.last_flow_moves.shape == (Mt, 1) and ais.last_flow_moves.is_cuda
