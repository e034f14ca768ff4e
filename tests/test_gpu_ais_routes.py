"""The routes into the fused AIS call when the noise is NOT passed in: the one-op call (`prefetch = False`), the two-piece call
with the next chain initialisation prefetched (`prefetch = True`), and the sharded backend stepped from Python on one process.
They draw eps0, the transition noise and nothing else from the device generator, in that order and with the same launches, so
after `torch.manual_seed(s)` on identically built samplers every route gives the same particles, log-weights, step sizes AND
leaves the generator in the same state.  (The sharded and SMC tests pass explicit noise; this file pins the draws.)

B = 200 is not a multiple of 16: the last tile of chains, and the last 16-chain block of the acceptance slab, are ragged."""
import pytest
import torch

pytestmark = pytest.mark.gpu
fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import parallel      # noqa: E402

DEV = "cuda"
D, K, NODES, M, L, B = 32, 3, 10, 4, 3, 200
SEED = 11


def _flow(seed=0):
    torch.manual_seed(seed)
    flow = fa.make_wrapped_normflow_realnvp(D, K, NODES, act_norm=False).to(DEV).requires_grad_(False)
    with torch.no_grad():
        for l1, l2, l3, aff in flow._layers():
            l3.weight.add_(0.01 * torch.randn_like(l3.weight))
    return flow


def _hmc_sampler():
    flow, target = _flow(), fa.ManyWellEnergy(D)
    hmc = fa.HamiltonianMonteCarlo(M, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.15, L=L).to(DEV)
    return fa.AnnealedImportanceSampler(flow, target.log_prob, hmc, False, 2.0, M), hmc


def _metropolis_sampler():
    flow, target = _flow(), fa.ManyWellEnergy(D)
    op = fa.Metropolis(M, D, flow.log_prob, target.log_prob, n_updates=2, alpha=2.0, p_target=False, max_step_size=0.4,
                       min_step_size=0.1, adjust_step_size=True).to(DEV)
    return fa.AnnealedImportanceSampler(flow, target.log_prob, op, False, 2.0, M), op


def _rng():
    return torch.cuda.get_rng_state(torch.cuda.current_device())


def _snap(pt, lw, step_state, rng):
    return [pt.x.clone(), pt.log_q.clone(), pt.log_p.clone(), lw.clone()] + [t.clone() for t in step_state] + [rng]


NAMES = ("x", "log_q", "log_p", "log_w", "step state 0", "step state 1", "generator state")


def _assert_same(ref, got, route):
    assert len(ref) == len(got) == 2
    for call, (ra, rb) in enumerate(zip(ref, got)):
        assert len(ra) == len(rb)
        for name, ta, tb in zip(NAMES, ra, rb):
            assert torch.equal(ta, tb), f"{route}: {name} of call {call} differs from the one-op call's"


def _fused_calls(prefetch):
    """Two consecutive `sample_and_log_weights(B)`.  With the prefetch on, the second call runs in two pieces and has drawn the
    THIRD call's eps0 by the time it returns: the state the call itself left is the one recorded in front of that draw (the
    state the sampler rewinds to when the third call turns out different), and nothing else has been drawn since."""
    ais, hmc = _hmc_sampler()
    ais.prefetch = prefetch
    torch.manual_seed(SEED)
    outs = []
    for call in range(2):
        pt, lw = ais.sample_and_log_weights(B)
        rng = _rng()
        pf = ais.__dict__.get("_pf_state")
        assert (pf is not None) == (prefetch and call == 1)
        if pf is not None:
            assert torch.equal(pf[3], rng)
            rng = pf[2]
        outs.append(_snap(pt, lw, (hmc.epsilons, hmc.common_epsilon), rng))
    return outs


def _stepped_shard_calls():
    """`HipShardBackend` on one process, the noise drawn by `_state`: begin, M x (step, adapt on its own slab), finish."""
    ais, hmc = _hmc_sampler()
    be = parallel.HipShardBackend(ais)
    torch.manual_seed(SEED)
    outs = []
    for call in range(2):
        st = be.begin(B)
        for j in range(1, M + 1):
            be.adapt(st, j, be.step(st, j), 1)
        pt, lw = be.finish(st)
        outs.append(_snap(pt, lw, (hmc.epsilons, hmc.common_epsilon), _rng()))
    return outs


@pytest.fixture(scope="module")
def one_op_calls():
    outs = _fused_calls(prefetch=False)
    assert outs[0][0].shape[1] == D and 0 < outs[0][0].shape[0] <= B and not torch.equal(outs[0][0], outs[1][0])
    assert not torch.equal(outs[0][4], outs[1][4])                          # tuning is on: the step sizes moved
    assert not torch.equal(outs[0][6], outs[1][6])
    return outs


def test_prefetched_two_piece_calls_draw_and_compute_what_the_one_op_calls_do(one_op_calls):
    _assert_same(one_op_calls, _fused_calls(prefetch=True), "prefetch")


def test_stepped_shard_backend_draws_and_computes_what_the_one_op_calls_do(one_op_calls):
    _assert_same(one_op_calls, _stepped_shard_calls(), "stepped shard backend")


def test_deferred_metropolis_call_draws_and_computes_what_the_one_op_call_does():
    """Metropolis, n_updates = 2, noise scalings adjusting: `run()` against `run_metropolis_deferred` + `adapt_metropolis` on one
    rank (the whole call through the phase op, the rule applied afterwards to the call's own slab)."""
    ais1, op1 = _metropolis_sampler()
    start = op1.noise_scalings.clone()
    torch.manual_seed(SEED)
    ref = []
    for call in range(2):
        pt, lw = ais1.sample_and_log_weights(B)
        ref.append(_snap(pt, lw, (op1.noise_scalings, op1.noise_scalings), _rng()))
    assert ref[0][0].shape[1] == D and 0 < ref[0][0].shape[0] <= B and not torch.equal(op1.noise_scalings, start)
    ais2, op2 = _metropolis_sampler()
    be = parallel.HipShardBackend(ais2)
    torch.manual_seed(SEED)
    got = []
    for call in range(2):
        pt, lw, slab = be.run_metropolis_deferred(B)
        be.adapt_metropolis(slab, 1, B)
        got.append(_snap(pt, lw, (op2.noise_scalings, op2.noise_scalings), _rng()))
    _assert_same(ref, got, "deferred Metropolis")
