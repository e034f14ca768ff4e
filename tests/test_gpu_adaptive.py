"""Adaptive annealing schedules on the GPU (distribution_spacing_type="adaptive", include/fabhip.h: fabhip_next_beta) against their
specification (tests/adaptive_spec.py), and custom schedules on the fused call.

G1  the decision kernel: every one of its four doubles EQUAL to the spec's, through the op and through the C ABI.
G2  whole calls, teacher-forced as in tests/test_gpu_smc.py: every recorded decision's own inputs go into the spec; the final
    log_w against the spec driver run on the device's schedule (and, with resampling on, on the device's log_w_pre).
G3  a forced linear schedule through the stepped driver is bit-identical to the fused call.
G4  custom schedules on the fused call.
G5  trainer smoke, evaluation data, logging keys, prefetch bypass, fast mode.

G2 - G4 use benign inputs in the sense of tests/test_gpu_smc.py (last coupling Linears N(0, 0.01^2), step 0.05): every accept margin
is far from its threshold, so a flipped accept decision is a failure - it would move x by a step, far outside RTOL."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import close, max_rel_err, seeded_oracle_flow, RTOL
import adaptive_spec
import smc_spec

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _lib, _ops            # noqa: E402
from oracle import ais as oais                  # noqa: E402
from oracle import targets as otgt              # noqa: E402

DEV = "cuda"
D, K, NODES, M, L, STEP = 6, 3, 10, 4, 3, 0.05


# ---- G1: the kernel against the spec -------------------------------------------------------------------------------------------------
def _case(n0, pad, scale, seed):
    g = np.random.default_rng(seed)
    B = n0 + pad
    lw = g.normal(size=B).astype(np.float32)
    lq = g.normal(size=B).astype(np.float32)
    lp = (lq + np.float32(scale) * g.normal(size=B).astype(np.float32)).astype(np.float32)
    if n0 >= 63:                                         # rows that weigh 0, wherever the bisection looks
        lw[5], lw[17], lw[n0 - 1], lp[40] = np.nan, np.inf, -np.inf, -np.inf
    for a in (lw, lq, lp):
        a[n0:] = np.nan                                  # never read: a row beyond n0 that entered a sum would poison it
    return lw, lq, lp


def _device_out4(lw, lq, lp, n0, beta, alpha, p_target, rho, use_n_valid):
    """(op, op again, C ABI) results as lists of 4 floats."""
    ops, lib = _ops.load(), _lib.load()
    t = [torch.from_numpy(a).to(DEV) for a in (lw, lq, lp)]
    nv = torch.tensor([n0, 0], dtype=torch.int32, device=DEV) if use_n_valid else None
    a = ops.next_beta(*t, nv, beta, alpha, p_target, rho)
    b = ops.next_beta(*t, nv, beta, alpha, p_target, rho, 24)
    out = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
    _lib.check(lib.fabhip_next_beta(_lib.ptr(t[0]), _lib.ptr(t[1]), _lib.ptr(t[2]), lw.shape[0], _lib.ptr(nv), C.c_double(beta),
                                    C.c_double(alpha), int(p_target), C.c_double(rho), 24, _lib.ptr(out), _lib.stream_ptr()),
               "next_beta")
    assert a.dtype == torch.float64 and a.shape == (4,)
    return a.cpu().tolist(), b.cpu().tolist(), out.cpu().tolist()


# around the wave and block sizes; 1025 / 2500 / 5000: more than one row per thread in registers; 8200: beyond the 8 x 1024 rows the
# kernel keeps in registers (its global-memory loop)
@pytest.mark.parametrize("n0", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2500, 5000, 8200])
def test_next_beta_equals_the_spec(n0):
    betas, combo, seen = [0.0, 0.25, 1 - 2.0 ** -20, 1.0], 0, set()
    for pad in (0, 7):
        for scale in (0.01, 5.0, 1e9):
            lw, lq, lp = _case(n0, pad, scale, seed=1000 + n0 + pad)
            for beta in betas:
                rho, p_target = (0.5, 0.9)[combo % 2], bool((combo // 2) % 2)      # (every pair of settings occurs over the loop)
                combo += 1
                want = adaptive_spec.next_beta(lw[:n0], lq[:n0], lp[:n0], beta, 2.0, p_target, rho)
                got = _device_out4(lw, lq, lp, n0, beta, 2.0, p_target, rho, use_n_valid=pad > 0)
                tag = f"n0={n0} B={n0 + pad} scale={scale} beta={beta} rho={rho} p_target={p_target}"
                assert got[0] == want.as_out4(), f"{tag}: op {got[0]} spec {want.as_out4()}"
                assert got[1] == got[0], f"{tag}: two launches differ"
                assert got[2] == got[0], f"{tag}: C ABI {got[2]} op {got[0]}"
                if beta == 0.0 and n0 >= 63:
                    seen.add((scale, want.evaluations, want.floor))
    if n0 >= 63:                                         # the three regimes were all met: immediate 1, interior, floor
        assert seen == {(0.01, 2, False), (5.0, 26, False), (1e9, 26, True)}, seen


@pytest.mark.parametrize("n0", [700, 5000])
@pytest.mark.parametrize("iters", [1, 2, 5, 24, 31])
def test_next_beta_with_other_iteration_counts(n0, iters):
    """K is the caller's: odd and even counts, one iteration, more than the default."""
    lw, lq, lp = _case(n0, 3, 5.0, seed=77 + n0)
    nv = torch.tensor([n0, 0], dtype=torch.int32, device=DEV)
    t = [torch.from_numpy(a).to(DEV) for a in (lw, lq, lp)]
    for beta, rho in ((0.0, 0.7), (0.4, 0.5)):
        want = adaptive_spec.next_beta(lw[:n0], lq[:n0], lp[:n0], beta, 2.0, False, rho, K=iters)
        got = _ops.load().next_beta(*t, nv, beta, 2.0, False, rho, iters).cpu().tolist()
        assert want.evaluations == 2 + iters and got == want.as_out4(), (beta, rho, got, want.as_out4())


def test_next_beta_rejects_bad_arguments():
    ops = _ops.load()
    t = torch.zeros(8, device=DEV)
    for beta, rho, iters in ((-0.1, 0.7, 24), (1.5, 0.7, 24), (0.0, 0.0, 24), (0.0, 1.0, 24), (0.0, 0.7, 0), (0.0, 0.7, 61),
                             (float("nan"), 0.7, 24)):
        with pytest.raises(RuntimeError):
            ops.next_beta(t, t, t, None, beta, 2.0, False, rho, iters)


# ---- samplers of G2 - G4 -------------------------------------------------------------------------------------------------------------
def hip_flow(nf, d=D, k=K, nodes=NODES):
    f = fa.RealNVP(d, k, nodes)
    f._nf_model.load_state_dict(nf.state_dict())
    return f.to(DEV).requires_grad_(False)


def inputs(B, seed=0, hmc=True, kill=()):
    g = torch.Generator().manual_seed(200 + seed)
    eps0 = torch.randn(B, D, generator=g)
    for r in kill:                                        # a chain the "chain init" filter removes (x = inf)
        eps0[r] = float("inf")
    n_inner = 1 if hmc else 2
    na = torch.randn(M, n_inner, B, D, generator=g)
    nb = torch.empty(M, n_inner, B).exponential_(1.0, generator=g) if hmc else torch.rand(M, n_inner, B, generator=g)
    nr = torch.rand(M, generator=g, dtype=torch.float64)
    return eps0, na, nb, nr


def samplers(hmc=True, eval_mode=True, **kw):
    nf = seeded_oracle_flow(D, K, NODES, 7, std=0.01)
    hf = hip_flow(nf)
    target = fa.ManyWellEnergy(D)
    if hmc:
        op = fa.HamiltonianMonteCarlo(M, D, hf.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=STEP, L=L,
                                      eval_mode=eval_mode).to(DEV)
    else:
        op = fa.Metropolis(M, D, hf.log_prob, target.log_prob, n_updates=2, alpha=2.0, p_target=False, max_step_size=0.05,
                           min_step_size=0.02, eval_mode=eval_mode).to(DEV)
    return nf, op, fa.AnnealedImportanceSampler(hf, target.log_prob, op, False, 2.0, M, **kw)


def oracle_sampler(nf, hmc, cls, **kw):
    ot = otgt.ManyWell(D)
    if hmc:
        op = oais.HMC(M, D, nf.log_prob, ot.log_prob, alpha=2.0, p_target=False, epsilon=STEP, L=L, eval_mode=True)
    else:
        op = oais.Metropolis(M, D, nf.log_prob, ot.log_prob, n_updates=2, alpha=2.0, p_target=False, max_step_size=0.05,
                             min_step_size=0.02, eval_mode=True)
    return cls(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, ot.log_prob, op, False, 2.0, M, **kw)


def step_state(op, hmc):
    return (op.epsilons.clone(), op.common_epsilon.clone()) if hmc else (op.noise_scalings.clone(),)


# ---- G2: whole calls, teacher-forced -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
@pytest.mark.parametrize("shape,B,kill,tau", [(16, 100, (), None), (8, 99, (), None), (4, 101, (), None), (4, 100, (3, 40), None),
                                              (16, 100, (), 0.5)])
def test_adaptive_call_follows_the_spec(shape, B, kill, tau, hmc):
    rho = 0.7
    eps0, na, nb, nr = inputs(B, seed=1, hmc=hmc, kill=kill)
    nf, op, ais = samplers(hmc=hmc, distribution_spacing_type="adaptive", ess_decay=rho, resample_threshold=tau)
    with _ops.option(_ops.OPT_TILE_SHAPE, shape):        # (the tile shape where the library has it for this flow, else its own choice)
        pt, log_w, n_valid, stats, _, _ = ais.run(B, eps0.to(DEV), na.to(DEV), nb.to(DEV), trace=True,
                                                  noise_r=nr.to(DEV) if tau is not None else None)
    n0, n1 = int(n_valid[0]), int(n_valid[1])
    assert n0 == n1 == B - len(kill)
    betas = ais.last_betas
    assert betas.dtype == torch.float64 and betas.shape == (M + 2,) and float(betas[0]) == 0.0 and float(betas[-1]) == 1.0
    assert bool((betas[1:] >= betas[:-1]).all()) and 0.0 < float(betas[1]) <= 1.0
    # every decision on the inputs the kernel saw
    assert [d.step for d in ais.last_adaptive] == list(range(len(ais.last_adaptive))) and 1 <= len(ais.last_adaptive) <= M
    for d in ais.last_adaptive:
        lw, lq, lp = (t[:n0].cpu().numpy() for t in d.inputs)
        want = adaptive_spec.next_beta(lw, lq, lp, d.beta, 2.0, False, rho)
        assert d.beta_next == want.beta_next, f"decision {d.step}: beta_next {d.beta_next} vs spec {want.beta_next}"
        assert (d.ess0, d.ess_choice, d.evaluations, d.floor) == (want.ess0, want.ess_choice, want.evaluations, want.floor)
        assert d.beta == float(betas[d.step]) and want.beta_next == float(betas[d.step + 1])
    # the call against the spec driver on the device's schedule, the same noise
    teacher = None
    if tau is not None:
        resampled, ess, anc, lw_pre = ais.last_smc
        teacher = [lw_pre[j][:n0].cpu().numpy() for j in range(M)]
    spec = oracle_sampler(nf, hmc, adaptive_spec.Adaptive, ess_decay=rho, resample_threshold=tau)
    ps, lws, info = spec.sample_and_log_weights(eps0, na, nb, noise_r=nr, force_betas=betas.tolist(), teacher_log_w_pre=teacher)
    if tau is not None:
        for j in range(M):
            assert bool(resampled[j]) == spec.trace.resampled[j], f"transition {j + 1}: the resampling decision differs"
            assert np.array_equal(anc[j][:n0].cpu().numpy().astype(np.int64), spec.trace.ancestors[j])
    assert ps.x.shape[0] == n1
    assert max_rel_err(pt.x[:n1], ps.x) <= RTOL, f"x err {max_rel_err(pt.x[:n1], ps.x):.2e}: an accept decision differs"
    assert close(pt.log_q[:n1], ps.log_q, RTOL) and close(pt.log_p[:n1], ps.log_p, RTOL)
    assert close(log_w[:n1], lws, RTOL, atol_scale=4), f"log_w err {max_rel_err(log_w[:n1], lws):.2e}"


# ---- G3: a forced linear schedule is the fused call ----------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
@pytest.mark.parametrize("B", [100, 1500])
def test_forced_linear_schedule_is_bit_identical_to_the_fused_call(B, hmc):
    eps0, na, nb, _ = inputs(B, seed=3, hmc=hmc, kill=(1,))
    runs = []
    for adaptive in (False, True):
        _, op, ais = samplers(hmc=hmc, eval_mode=False, distribution_spacing_type="adaptive" if adaptive else "linear")
        kw = dict(force_betas=ais.B_space.clone()) if adaptive else {}
        pt, log_w, n_valid, stats, _, _ = ais.run(B, eps0.to(DEV), na.to(DEV), nb.to(DEV), **kw)
        runs.append((pt.x, pt.log_q, pt.log_p, log_w, n_valid.clone(), stats[:6].clone(), *step_state(op, hmc)))
        if adaptive:
            assert torch.equal(ais.last_betas, ais.B_space) and len(ais.last_adaptive) == M
    n1 = int(runs[0][4][1])
    assert n1 == B - 1
    cut = lambda t: t[:n1] if t.dim() >= 1 and t.shape[0] == B else t      # noqa: E731
    names = ("x", "log_q", "log_p", "log_w", "n_valid", "stats", "step sizes", "common step size")
    for name, u, v in zip(names, *runs):
        assert torch.equal(cut(u), cut(v)), f"{name} differs between the fused call and the stepped driver"


# ---- G4: custom schedules on the fused call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hmc", [True, False])
def test_custom_schedule_equal_to_linear_is_bit_identical(hmc):
    B = 200
    eps0, na, nb, _ = inputs(B, seed=4, hmc=hmc, kill=(7,))
    runs = []
    for spacing in ("linear", np.linspace(0.0, 1.0, M + 2).tolist()):
        _, op, ais = samplers(hmc=hmc, eval_mode=False, distribution_spacing_type=spacing)
        pt, log_w, n_valid, stats, _, _ = ais.run(B, eps0.to(DEV), na.to(DEV), nb.to(DEV))
        runs.append((pt.x, pt.log_q, pt.log_p, log_w, n_valid.clone(), stats[:6].clone(), *step_state(op, hmc)))
    n1 = int(runs[0][4][1])
    cut = lambda t: t[:n1] if t.dim() >= 1 and t.shape[0] == B else t      # noqa: E731
    assert n1 == B - 1 and all(torch.equal(cut(u), cut(v)) for u, v in zip(*runs))


@pytest.mark.parametrize("hmc", [True, False])
def test_custom_schedule_with_a_repeated_entry_follows_the_oracle(hmc):
    B = 150
    sched = [0.0, 0.01, 0.1, 0.1, 0.4, 1.0]              # geometric-like, one step without an increment
    eps0, na, nb, _ = inputs(B, seed=5, hmc=hmc)
    nf, op, ais = samplers(hmc=hmc, distribution_spacing_type=torch.tensor(sched, dtype=torch.float64))
    pt, log_w = ais.sample_and_log_weights(B, eps0=eps0.to(DEV), noise_a=na.to(DEV), noise_b=nb.to(DEV))
    ref = oracle_sampler(nf, hmc, oais.AIS)
    ref.B_space = torch.tensor(sched, dtype=torch.float64)
    po, lwo, info = ref.sample_and_log_weights(eps0, na, nb)
    assert max_rel_err(pt.x, po.x) <= RTOL and close(pt.log_q, po.log_q, RTOL) and close(pt.log_p, po.log_p, RTOL)
    assert close(log_w, lwo, RTOL), f"log_w err {max_rel_err(log_w, lwo):.2e}"
    assert abs(ais.get_logging_info()["log_Z"] - info.log_Z) <= 1e-4 * max(1.0, abs(info.log_Z))


# ---- G5: trainer smoke + the Python surface ---------------------------------------------------------------------------------------------
def test_trainer_runs_on_an_adaptive_schedule():
    Dt, Mt, B = 6, 4, 256
    torch.manual_seed(1)
    flow = fa.make_wrapped_normflow_realnvp(Dt, 4, 10, act_norm=False).to(DEV)
    target = fa.ManyWellEnergy(Dt)
    hmc = fa.HamiltonianMonteCarlo(Mt, Dt, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.2, L=5).to(DEV)
    model = fa.FABModel(flow, target, Mt, alpha=2.0, transition_operator=hmc, loss_type="fab_alpha_div",
                        ais_distribution_spacing="adaptive", ais_ess_decay=0.6)
    ais = model.annealed_importance_sampler
    assert ais.adaptive and ais.ess_decay == 0.6

    def initial_sampler():
        pt, lw = ais.sample_and_log_weights(B, logging=False)
        return pt.x, lw, pt.log_q
    buf = fa.PrioritisedReplayBuffer(Dt, 8 * B, 2 * B, initial_sampler, device=DEV)
    opt = fa.FlatAdam(flow, lr=1e-4)
    trainer = fa.PrioritisedBufferTrainer(model, opt, buf, alpha=2.0, n_batches_buffer_sampling=2)
    for i in range(3):
        info = trainer.step(i, B)
        assert np.isfinite(info["loss"]), (i, info)
        assert 0.0 < info["beta_1"] <= 1.0 and 1 <= info["n_steps_to_beta_one"] <= Mt + 1 and 0 <= info["n_bisect_floor"] <= Mt
        assert 0 < info["ess_ais"] <= 1 and np.isfinite(info["log_Z"])
        b = ais.last_betas
        assert b.shape == (Mt + 2,) and float(b[0]) == 0.0 and float(b[-1]) == 1.0 and bool((b[1:] >= b[:-1]).all())
    assert torch.isfinite(buf.buffer.log_w[:buf.current_index]).all() and torch.isfinite(buf.buffer.x[:buf.current_index]).all()
    bx, blw, ax, alw = ais.generate_eval_data(2 * B, B)
    assert bx.shape == ax.shape == (2 * B, Dt) and blw.shape == alw.shape == (2 * B,)
    assert torch.isfinite(alw).all() and torch.isfinite(blw).all()


def test_logging_keys_prefetch_bypass_resampling_and_fast_mode():
    B = 128
    _, op, ais = samplers()
    torch.manual_seed(0)
    for _ in range(3):
        ais.sample_and_log_weights(B)
    assert "_pf_state" in ais.__dict__ and "beta_1" not in ais.get_logging_info()
    ais.distribution_spacing_type = "adaptive"           # settable; the prefetched piece is dropped, the mode's calls are stepped
    for _ in range(2):
        pt, lw = ais.sample_and_log_weights(B)
    info = ais.get_logging_info()
    assert "_pf_state" not in ais.__dict__ and {"beta_1", "n_steps_to_beta_one", "n_bisect_floor"} <= set(info)
    assert torch.isfinite(lw).all() and pt.x.shape == (B, D) and 0 < info["ess_ais"] <= 1
    # with resampling on, either method, and Metropolis
    for method in ("systematic", "stratified"):
        ais.resample_threshold, ais.resample_method = 1.5, method
        pt, lw = ais.sample_and_log_weights(B)
        info = ais.get_logging_info()
        assert info["n_resampled"] == M and torch.isfinite(lw).all() and float(ais.last_betas[-1]) == 1.0
    _, _, met = samplers(hmc=False, distribution_spacing_type="adaptive", ess_decay=0.5)
    pt, lw = met.sample_and_log_weights(B)
    assert torch.isfinite(lw).all() and pt.grad_log_q is None and float(met.last_betas[-1]) == 1.0
    # precision="fast" (bf16 conditioner GEMMs) on the headline architecture's width
    nf = seeded_oracle_flow(32, 3, 10, 7, std=0.01)
    hf = hip_flow(nf, 32, 3, 10)
    hf.precision = "fast"
    target = fa.ManyWellEnergy(32)
    hop = fa.HamiltonianMonteCarlo(M, 32, hf.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=STEP, L=L).to(DEV)
    fast = fa.AnnealedImportanceSampler(hf, target.log_prob, hop, False, 2.0, M, distribution_spacing_type="adaptive")
    pt, lw = fast.sample_and_log_weights(B)
    assert torch.isfinite(lw).all() and pt.x.shape == (B, 32) and float(fast.last_betas[-1]) == 1.0
    # force_betas belongs to the adaptive mode
    with pytest.raises(_ops.FabhipError, match="force_betas"):
        samplers()[2].run(B, force_betas=[0.0, 0.2, 0.4, 0.6, 0.8, 1.0])
