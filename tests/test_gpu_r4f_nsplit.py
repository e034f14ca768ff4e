"""N-split hidden-width products of the fused 4-chain kernels (flow_r4f.h, density direction, fp32 path): lane quarter Q of
every wave multiplies the K range wave Q used to multiply, for the 16 G columns its wave owns, and the four quarters are added
inside the wave as (P0 + P1) + (P2 + P3) - the sums the K-split stages formed through LDS, in the same order.  Everything a fused
AIS call returns therefore stays bit-identical to what the K-split kernels returned (tests/golden/g20_r4f_nsplit.npz, recorded
by tools/record_r4f_nsplit.py on the commit before the change), agrees with the oracle, and repeated launches agree bit for bit
(a missing barrier shows as non-determinism).  Fast mode keeps the K-split stages and its own image: bit-identical as well.

Shapes: (D, nodes) = (32, 10), (32, 4), (6, 40): G = hidden width / 64 = 5, 2, and 4 with d = 3; K = 3 (an interior layer on both
sweeps), M = L = 2; B = 4 (one workgroup) and B = 7 (a partial last workgroup); a tuned and a frozen-step-size call each."""
import os

import numpy as np
import pytest
import torch

from helpers import close, max_rel_err, RTOL, GOLDEN, seeded_oracle_flow

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops            # noqa: E402
from oracle import ais as oais            # noqa: E402
from oracle import targets as otgt        # noqa: E402

DEV = "cuda"
FIXTURE = "g20_r4f_nsplit.npz"
K, M, L = 3, 2, 2
SHAPES = [(32, 10), (32, 4), (6, 40)]                   # G = 5, 2 and G = 4 with d = 3
CASES = [(D, nodes, B, ev) for D, nodes in SHAPES for B in (4, 7) for ev in (False, True)]
FAST_CASES = [(32, 10, 7, False), (32, 10, 7, True)]
REPEATED = (32, 10, 7, False)


def case_key(D, nodes, B, ev, fast=False):
    return f"D{D}_n{nodes}_B{B}_{'eval' if ev else 'tuned'}" + ("_fast" if fast else "")


_flows = {}


def flows_of(D, nodes):
    """(oracle flow, its HIP twin) of a shape: seeded, built once per session."""
    if (D, nodes) not in _flows:
        nf = seeded_oracle_flow(D, K, nodes, 200 + D + nodes)
        hf = fa.RealNVP(D, K, nodes)
        hf._nf_model.load_state_dict(nf.state_dict())
        _flows[(D, nodes)] = (nf, hf.to(DEV).requires_grad_(False))
    return _flows[(D, nodes)]


def noise_of(D, B):
    g = torch.Generator().manual_seed(2000 + 10 * D + B)
    eps0 = torch.randn(B, D, generator=g)
    noise_p = torch.randn(M, 1, B, D, generator=g)
    noise_e = torch.empty(M, 1, B).exponential_(generator=g)
    return eps0, noise_p, noise_e


def ais_call(D, nodes, B, eval_mode=False, fast=False, shape=4):
    """One fused AIS call (step-size tuning on unless eval_mode) on seeded noise with the tile shape forced.
    Returns dict(x, log_w, log_q, grad_log_q, epsilons, common_epsilon) of CPU tensors."""
    _, hf = flows_of(D, nodes)
    target = fa.ManyWellEnergy(D)
    eps0, noise_p, noise_e = noise_of(D, B)
    hmc = fa.HamiltonianMonteCarlo(M, D, hf.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.12, L=L,
                                   eval_mode=eval_mode).to(DEV)
    ais = fa.AnnealedImportanceSampler(hf, target.log_prob, hmc, False, 2.0, M)
    with _ops.option(_ops.OPT_TILE_SHAPE, shape), fa.fast_mode(fast):
        pt, lw = ais.sample_and_log_weights(B, eps0=eps0.to(DEV), noise_a=noise_p.to(DEV), noise_b=noise_e.to(DEV))
    return dict(x=pt.x.cpu(), log_w=lw.cpu(), log_q=pt.log_q.cpu(), grad_log_q=pt.grad_log_q.cpu(),
                epsilons=hmc.epsilons.detach().cpu().clone(), common_epsilon=hmc.common_epsilon.detach().cpu().reshape(-1).clone())


def weight_probe(D, nodes):
    nf, _ = flows_of(D, nodes)
    return torch.cat([nf.flows[0].flows[1].param_map.net[2].weight[0, :8].detach(),
                      nf.flows[-2].flows[1].param_map.net[4].weight[1, :4].detach(),
                      noise_of(D, 7)[0][0, :4]]).numpy()


RECORDED = ("x", "log_w", "log_q", "grad_log_q", "epsilons", "common_epsilon")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, FIXTURE), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def calls():
    """The call at tile shape 4 of every fp32 case, computed once."""
    return {c: ais_call(c[0], c[1], c[2], eval_mode=c[3]) for c in CASES}


@pytest.mark.parametrize("D,nodes,B,ev", CASES)
def test_fused_ais_call_is_bit_identical_to_the_k_split_kernels(golden, calls, D, nodes, B, ev):
    assert np.array_equal(weight_probe(D, nodes), golden[f"probe_D{D}_n{nodes}"]), \
        "the seeded flow / noise differs from what the fixture was recorded with"
    for name in RECORDED:
        np.testing.assert_array_equal(calls[(D, nodes, B, ev)][name].numpy(), golden[f"{case_key(D, nodes, B, ev)}.{name}"],
                                      err_msg=name)


@pytest.mark.parametrize("D,nodes,B,ev", FAST_CASES)
def test_fast_mode_is_untouched(golden, D, nodes, B, ev):
    r = ais_call(D, nodes, B, eval_mode=ev, fast=True)
    for name in RECORDED:
        np.testing.assert_array_equal(r[name].numpy(), golden[f"{case_key(D, nodes, B, ev, fast=True)}.{name}"], err_msg=name)


def test_ten_repeated_launches_are_bitwise_equal(calls):
    D, nodes, B, ev = REPEATED
    first = calls[REPEATED]
    for rep in range(10):
        again = ais_call(D, nodes, B, eval_mode=ev)
        for name, v in first.items():
            assert torch.equal(v, again[name]), f"launch {rep + 1}: {name} differs"


@pytest.mark.parametrize("D,nodes,B,ev", CASES)
def test_fused_ais_call_matches_the_oracle(calls, D, nodes, B, ev):
    nf, _ = flows_of(D, nodes)
    r4 = calls[(D, nodes, B, ev)]
    eps0, noise_p, noise_e = noise_of(D, B)
    ot = otgt.ManyWell(D)
    ohmc = oais.HMC(M, D, nf.log_prob, ot.log_prob, alpha=2.0, p_target=False, epsilon=0.12, L=L, eval_mode=ev)
    oa = oais.AIS(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, ot.log_prob, ohmc, False, 2.0, M)
    opt, olw, _ = oa.sample_and_log_weights(eps0, noise_p, noise_e)
    x, lw, lq, gq = opt.x.detach(), olw.detach(), opt.log_q.detach(), opt.grad_log_q.detach()
    scale = max(1.0, float(x.abs().max()))
    err = (r4["x"] - x).abs().max(1).values / scale
    print(f"{case_key(D, nodes, B, ev)} vs oracle: x err {float(err.max()):.2e}  log_w err {max_rel_err(r4['log_w'], lw):.2e}  "
          f"log_q err {max_rel_err(r4['log_q'], lq):.2e}  grad err {max_rel_err(r4['grad_log_q'], gq):.2e}")
    # the bounds of tests/test_gpu_r4f_handover.py: 1e-4 of the state scale; one chain may differ through an accept decision
    # within rounding of its threshold (it then differs as a whole and is left out of the other comparisons)
    flipped = err > 1e-4
    assert int(flipped.sum()) <= 1, f"{int(flipped.sum())} chains differ (max err {float(err.max()):.2e})"
    ok = ~flipped
    assert close(r4["log_w"][ok], lw[ok], RTOL), f"log_w err {max_rel_err(r4['log_w'][ok], lw[ok]):.2e}"
    assert close(r4["log_q"][ok], lq[ok], RTOL), f"log_q err {max_rel_err(r4['log_q'][ok], lq[ok]):.2e}"
    assert close(r4["grad_log_q"][ok], gq[ok], 5e-4), f"grad err {max_rel_err(r4['grad_log_q'][ok], gq[ok]):.2e}"
