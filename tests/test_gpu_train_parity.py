"""GPU tests of PrioritisedBufferTrainer against the reference trainer's traces at the widths whose tape kernel carries the
minibatch arithmetic in its tail (g18: D = 32, 10 layers, W = 320 - the benchmarked shape, k_flow_log_prob_tape_r8<5> - in a mild
and a clipping regime; D = 6, W = 240, the <4> instantiation).  `flat_adam` is the one-op path with the tail
(`fabhip::buffer_train_step`), `torch_adam` autograd through the tape kernel the shape selects, without the tail.  The fixtures
hold no parameters: the flow is seeded, and the start-of-iteration states of the teacher-forced test (parameters, both Adam
moments, step sizes, buffer) come from oracle/train.py run inside the test, after its parameter probes matched the fixture
(tests/test_oracle_golden.py pins every other value of the oracle's replay to the trace)."""
import numpy as np
import pytest
import torch

from helpers import load_golden, close, worst, RTOL, g18_oracle_replay, probes_close, param_probes, flow_from_g14
from test_gpu_parity import hip_flow_from_oracle, DEV

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops            # noqa: E402

MILD = ("g18_trainer_w320_mild", "g18_trainer_w256_mild")
ALL = ("g18_trainer_w320_mild", "g18_trainer_w320_clip", "g18_trainer_w256_mild")
MINIBATCH_KEYS = ("loss", "grad_norm", "w_adjust_mean", "w_adjust_min", "w_adjust_max", "log_q_x_mean")


def _assert_path(g, optimiser, trainer):
    """The one-op step with the fused tail is what `flat_adam` runs here (and g12's shape would not): the dispatcher's own answer."""
    D, K, W = int(g["D"]), int(g["K"]), int(g["D"]) * int(g["nodes"])
    plan = [int(v) for v in _ops.load().train_step_plan(D, K, W)]
    assert plan == [8, 5 if W > 256 else 4, 1], plan
    assert [int(v) for v in _ops.load().train_step_plan(6, 3, 30)][2] == 0          # g12's shape: no tail
    for mode in (8, 16):
        with _ops.option(_ops.OPT_TAPE_TILES, mode):
            assert [int(v) for v in _ops.load().train_step_plan(D, K, W)][2] == 0
    assert (trainer._fused and trainer._one_op_minibatch()) == (optimiser == "flat_adam")


def _setup(g, optimiser):
    D, M, L, B = int(g["D"]), int(g["M"]), int(g["L"]), int(g["B"])
    alpha, n_batches = float(g["alpha"]), int(g["n_batches"])
    hf = hip_flow_from_oracle(flow_from_g14(g)).requires_grad_(True)
    target = fa.ManyWellEnergy(D)
    hmc = fa.HamiltonianMonteCarlo(M, D, hf.log_prob, target.log_prob, alpha=alpha, p_target=False, epsilon=float(g["eps_init"]),
                                   L=L).to(DEV)
    model = fa.FABModel(hf, target, M, alpha=alpha, transition_operator=hmc)
    ais = model.annealed_importance_sampler
    T = lambda k: torch.tensor(g[k]).to(DEV)          # noqa: E731
    calls = iter(range(int(g["n_init_calls"])))

    def initial_sampler():
        c = next(calls)
        pt, lw = ais.sample_and_log_weights(B, logging=False, eps0=T(f"call{c}_eps0"), noise_a=T(f"call{c}_noise_p"),
                                            noise_b=T(f"call{c}_noise_e"))
        assert close(lw, g[f"call{c}_log_w"], RTOL), f"initial call {c}: {worst(lw, g[f'call{c}_log_w']):.2f}x tol"
        return pt.x, lw, pt.log_q
    buf = fa.PrioritisedReplayBuffer(D, int(g["buf_len"]), int(g["buf_min"]), initial_sampler, device=DEV)
    opt = (torch.optim.Adam(hf.parameters(), lr=float(g["lr"])) if optimiser == "torch_adam" else fa.FlatAdam(hf, lr=float(g["lr"])))
    trainer = fa.PrioritisedBufferTrainer(model, opt, buf, alpha=alpha, n_batches_buffer_sampling=n_batches,
                                          max_gradient_norm=float(g["max_gradient_norm"]),
                                          w_adjust_max_clip=float(g["w_adjust_max_clip"]))
    _assert_path(g, optimiser, trainer)
    return hf, hmc, buf, opt, trainer, T


def _step(g, trainer, it, T):
    c = int(g["n_init_calls"]) + it
    ref_idx = torch.tensor(g[f"it{it}_indices"])
    order = torch.searchsorted(ref_idx.sort().values, ref_idx)      # reference order as positions in the sorted set
    info = trainer.step(it + 1, int(g["B"]), noise=dict(eps0=T(f"call{c}_eps0"), noise_a=T(f"call{c}_noise_p"),
                                                         noise_b=T(f"call{c}_noise_e"), gumbel=T(f"it{it}_gumbel"), perm=order.to(DEV)))
    assert torch.equal(trainer.last_indices.cpu(), ref_idx), f"iteration {it}: the sampled set or its order differs"
    return info


def _minibatch_values(trainer, j):
    """The scalars of minibatch j of the last iteration (host floats on every path)."""
    return trainer.minibatch_stats()[j]


def _named_params(hf, names):
    sd = dict(hf._nf_model.named_parameters())
    return [sd[n].detach() for n in names]


@pytest.mark.parametrize("optimiser", ["torch_adam", "flat_adam"])
@pytest.mark.parametrize("name", MILD)
def test_trainer_replays_the_wide_reference_traces_free_running(name, optimiser):
    """Free-running over the three iterations of the mild traces, with the assertions and tolerances of the g12 replay
    (test_gpu_workloads.py::test_trainer_replays_reference_traces): index set and order exact, scalars 2e-4, the buffer at 1e-4 in
    iteration 1 and 5e-4 after, final parameters (probes of every tensor) at the g12 test's 2e-5 + 1e-4 max|p| criterion."""
    g = load_golden(name + ".npz")
    hf, hmc, buf, opt, trainer, T = _setup(g, optimiser)
    n_iter, n_batches = int(g["n_iter"]), int(g["n_batches"])
    for it in range(n_iter):
        info = _step(g, trainer, it, T)
        for key in ("loss", "grad_norm", "ess_ais", "log_Z", "w_adjust_mean", "log_q_x_mean"):
            ref = float(g[f"it{it}_{key}"])
            assert abs(info[key] - ref) <= 2e-4 * max(1.0, abs(ref)), (it, key, info[key], ref)
        for j in range(n_batches):
            got = _minibatch_values(trainer, j)
            for key in MINIBATCH_KEYS:
                ref = float(g[f"it{it}_mb{j}_{key}"])
                assert abs(got[key] - ref) <= 2e-4 * max(1.0, abs(ref)), (it, j, key, got[key], ref)
        tol = RTOL if it == 0 else 5e-4
        assert close(buf.buffer.log_w, g[f"it{it}_buf_log_w"], tol), (it, worst(buf.buffer.log_w, g[f"it{it}_buf_log_w"], tol))
        assert close(buf.buffer.log_q_old, g[f"it{it}_buf_log_q_old"], tol), (it, worst(buf.buffer.log_q_old, g[f"it{it}_buf_log_q_old"], tol))
    np.testing.assert_allclose(hmc.epsilons.cpu().numpy(), g["out_epsilons"], rtol=1e-6)
    names = [n for n, _ in flow_from_g14(g).named_parameters()]
    got = param_probes(_named_params(hf, names), int(g["probe_seed"]))
    for i, (a, b, p_) in enumerate(zip(got, g["final_param_probe"], _named_params(hf, names))):
        # (max|p| of the g12 criterion is taken over the reference's probed entries: never larger than the tensor's own)
        tol = 2e-5 + 1e-4 * float(np.abs(b[:-2]).max())
        assert float(np.abs(a[:-2] - b[:-2]).max()) <= tol, (names[i], a[:-2], b[:-2])
        # the whole tensor through its stored sum and squared norm, at what the per-entry criterion implies for them:
        # |sum a - sum b| <= n tol;  | |a|^2 - |b|^2 | <= 2 |b| |a - b| + |a - b|^2 with |a - b| <= sqrt(n) tol
        n = p_.numel()
        assert abs(a[-2] - b[-2]) <= n * tol, (names[i], "sum", a[-2], b[-2])
        assert abs(a[-1] - b[-1]) <= 2 * np.sqrt(b[-1] * n) * tol + n * tol * tol, (names[i], "squared norm", a[-1], b[-1])


@pytest.mark.parametrize("optimiser", ["torch_adam", "flat_adam"])
@pytest.mark.parametrize("name", ALL)
def test_trainer_iterations_from_the_reference_state_at_the_wide_shapes(name, optimiser):
    """Teacher-forced: EVERY iteration restarts from the reference's state - taken from oracle/train.py's replay of the trace, whose
    parameter probes are first checked against the fixture - and ONE iteration is compared: sampled index set and order, every
    per-minibatch scalar at 1e-4 x max(1, |ref|), the buffer after the adjust and BOTH Adam moments in full at `helpers.close`
    1e-4, all parameters at 2e-6 + 1e-4 max|p| per tensor.
    Reference-side gaps these bounds were set from (float32 trace against a float64 oracle restarted from the same state, mild /
    clipping trace): scalars at most 1.5e-6 / 9.4e-6 relative; buffer 0.007 / 0.08 of the criterion; moments 0.14 / 0.20 of it.
    Parameters, iteration 1 only: the first two Adam steps from zero moments move an entry by about lr x sign(g), so an entry whose
    gradient is within rounding of zero lands elsewhere (the float64 oracle alone: 3 / 55 of 1 205 184 entries outside): at most
    1e-4 of all entries (120 at D = 32) may lie outside, each still within Adam's step bound n_minibatches x lr x (1 + 1e-3) of its
    start value; the count is printed.  Iterations 2 and 3: no entry outside."""
    g = load_golden(name + ".npz")
    seed, n_iter, n_batches, lr = int(g["probe_seed"]), int(g["n_iter"]), int(g["n_batches"]), float(g["lr"])
    r = g18_oracle_replay(g)
    names = [n for n, _ in r["nf"].named_parameters()]
    states = r["starts"] + [r["final"]]
    for it, st in enumerate(states):                       # the oracle's states are the reference's (probes of the fixture)
        ref = g[f"it{it}_param_probe"] if it < n_iter else g["final_param_probe"]
        assert probes_close([st["params"][n] for n in names], seed, ref, 1e-5) == [], it
    hf, hmc, buf, opt, trainer, T = _setup(g, optimiser)
    params = list(hf.parameters())
    hip_names = {id(p): n for n, p in hf._nf_model.named_parameters()}
    index = {n: i for i, n in enumerate(names)}

    def restore(it):
        st = states[it]
        with torch.no_grad():
            for k, p_ in hf._nf_model.state_dict().items():
                p_.copy_(st["params"][k].to(DEV))         # in place: FlatAdam's parameters are views of its flat buffer
            hmc.epsilons.copy_(st["eps"].to(DEV)); hmc.common_epsilon.copy_(st["ceps"].to(DEV))
            buf.buffer.x.copy_(st["buf_x"].to(DEV)); buf.buffer.log_w.copy_(st["buf_log_w"].to(DEV))
            buf.buffer.log_q_old.copy_(st["buf_log_q_old"].to(DEV))
            buf.current_index, buf.is_full = int(st["buf_index"]), bool(st["buf_full"])
            trainer._last_grad_norm = st["grad_norm"] if st["grad_norm"] is None else float(st["grad_norm"])
            if optimiser == "torch_adam":
                opt.state.clear()
                if st["adam"] is not None:
                    for p_ in params:
                        m_, v_, step = st["adam"][index[hip_names[id(p_)]]]
                        opt.state[p_] = {"step": torch.tensor(step), "exp_avg": m_.to(DEV).clone(), "exp_avg_sq": v_.to(DEV).clone()}
            else:
                opt.m.zero_(); opt.v.zero_(); opt.steps.zero_()
                if st["adam"] is not None:
                    for mv, which in ((opt.m, 0), (opt.v, 1)):
                        for view, p_ in zip(hf._grad_views(mv), hf._grad_tensors()):
                            view.copy_(st["adam"][index[hip_names[id(p_)]]][which].to(DEV).reshape(view.shape))
                    opt.steps.fill_(int(st["adam"][0][2]))
        hf._packed_key = None

    def moments():
        """{name: (exp_avg, exp_avg_sq)} on the host, and the step count."""
        if optimiser == "torch_adam":
            return ({hip_names[id(p_)]: (opt.state[p_]["exp_avg"].cpu(), opt.state[p_]["exp_avg_sq"].cpu()) for p_ in params},
                    int(float(opt.state[params[0]]["step"])))
        ms = {hip_names[id(p_)]: v.cpu() for v, p_ in zip(hf._grad_views(opt.m), hf._grad_tensors())}
        vs = {hip_names[id(p_)]: v.cpu() for v, p_ in zip(hf._grad_views(opt.v), hf._grad_tensors())}
        return {n: (ms[n], vs[n]) for n in ms}, int(opt.steps.item())
    for it in range(n_iter):
        restore(it)
        _step(g, trainer, it, T)
        for j in range(n_batches):
            got = _minibatch_values(trainer, j)
            for key in MINIBATCH_KEYS:
                ref = float(g[f"it{it}_mb{j}_{key}"])
                assert abs(got[key] - ref) <= RTOL * max(1.0, abs(ref)), (it, j, key, got[key], ref)
        assert close(buf.buffer.log_w, g[f"it{it}_buf_log_w"], RTOL), (it, worst(buf.buffer.log_w, g[f"it{it}_buf_log_w"]))
        assert close(buf.buffer.log_q_old, g[f"it{it}_buf_log_q_old"], RTOL), (it, worst(buf.buffer.log_q_old, g[f"it{it}_buf_log_q_old"]))
        nxt = states[it + 1]
        got_mv, steps = moments()
        assert steps == int(nxt["adam"][0][2]) == n_batches * (it + 1)
        for n in names:
            m_ref, v_ref, _ = nxt["adam"][index[n]]
            assert close(got_mv[n][0].reshape(m_ref.shape), m_ref, RTOL), (it, n, "exp_avg", worst(got_mv[n][0].reshape(m_ref.shape), m_ref))
            assert close(got_mv[n][1].reshape(v_ref.shape), v_ref, RTOL), (it, n, "exp_avg_sq", worst(got_mv[n][1].reshape(v_ref.shape), v_ref))
        outside, total = 0, 0
        for n, p_ in hf._nf_model.named_parameters():
            ref, start = nxt["params"][n], states[it]["params"][n]
            err = (p_.detach().cpu() - ref).abs()
            out = err > 2e-6 + RTOL * float(ref.abs().max())
            outside += int(out.sum()); total += ref.numel()
            if bool(out.any()):
                assert it == 0, (it, n, int(out.sum()), float(err.max()))
                assert float((p_.detach().cpu() - start).abs()[out].max()) <= n_batches * lr * (1 + 1e-3), (it, n)
        print(f"TEACHER-FORCED {name} {optimiser} iteration {it}: {outside} of {total} parameter entries outside 2e-6 + 1e-4 max|p|")
        assert outside <= (total // 10000 if it == 0 else 0), (it, outside, total)
