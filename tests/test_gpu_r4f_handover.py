"""In-wave hand-over of the fused 4-chain stages (flow_r4f.h): a wide stage's epilogue reduces, on every wave, exactly the
4 x 16 G outputs that wave's K range of the next stage reads, so S1 -> S2, S2 -> S3, S4 -> S5 and S5 -> S6 (and the sampling
direction's S1 -> S2 -> S3) need ONE workgroup barrier per stage, with the partial sums double-buffered.  Same sums in the same
order: everything a tuned AIS call returns is bit-identical to what the two-barrier kernels returned
(tests/golden/g19_r4f_handover.npz, recorded by tools/record_r4f_handover.py before the change), agrees with the oracle and
the 16-chain tiles, and repeated launches agree bit for bit (a missing barrier shows as non-determinism).

Shapes: (D, nodes) with G = hidden width / 64 = 2, 4, 5 column groups per wave and d = 3 (a K range of the narrow stages that
is no multiple of 16); K = M = L = 2; B = 4 (one workgroup) and B = 7 (a partial last workgroup)."""
import os

import numpy as np
import pytest
import torch

from helpers import close, max_rel_err, RTOL, GOLDEN, seeded_oracle_flow

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops            # noqa: E402
from oracle import ais as oais            # noqa: E402
from oracle import flow as oflow          # noqa: E402
from oracle import targets as otgt        # noqa: E402

DEV = "cuda"
FIXTURE = "g19_r4f_handover.npz"
K, M, L = 2, 2, 2
SHAPES = [(32, 4), (32, 8), (32, 10), (6, 40)]          # G = 2, 4, 5 and G = 4 with d = 3
CASES = [(D, nodes, B) for D, nodes in SHAPES for B in (4, 7)]


def case_key(D, nodes, B):
    return f"D{D}_n{nodes}_B{B}"


_flows = {}


def flows_of(D, nodes):
    """(oracle flow, its HIP twin) of a shape: seeded, built once per session."""
    if (D, nodes) not in _flows:
        nf = seeded_oracle_flow(D, K, nodes, 190 + D + nodes)
        hf = fa.RealNVP(D, K, nodes)
        hf._nf_model.load_state_dict(nf.state_dict())
        _flows[(D, nodes)] = (nf, hf.to(DEV).requires_grad_(False))
    return _flows[(D, nodes)]


def noise_of(D, B):
    g = torch.Generator().manual_seed(1900 + 10 * D + B)
    eps0 = torch.randn(B, D, generator=g)
    noise_p = torch.randn(M, 1, B, D, generator=g)
    noise_e = torch.empty(M, 1, B).exponential_(generator=g)
    return eps0, noise_p, noise_e


def ais_call(D, nodes, B, shape=4, eval_mode=False, fast=False):
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


RECORDED = ("x", "log_w", "log_q", "epsilons", "common_epsilon")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, FIXTURE), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tuned():
    """The tuned call at tile shape 4 of every case, computed once."""
    return {c: ais_call(*c) for c in CASES}


@pytest.mark.parametrize("D,nodes,B", CASES)
def test_tuned_ais_call_is_bit_identical_to_the_two_barrier_kernels(golden, tuned, D, nodes, B):
    assert np.array_equal(weight_probe(D, nodes), golden[f"probe_D{D}_n{nodes}"]), \
        "the seeded flow / noise differs from what the fixture was recorded with"
    for name in RECORDED:
        np.testing.assert_array_equal(tuned[(D, nodes, B)][name].numpy(), golden[f"{case_key(D, nodes, B)}.{name}"], err_msg=name)


@pytest.mark.parametrize("D,nodes,B", CASES)
def test_frozen_step_size_call_matches_the_oracle_and_the_sixteen_chain_tiles(D, nodes, B):
    nf, _ = flows_of(D, nodes)
    r4 = ais_call(D, nodes, B, shape=4, eval_mode=True)
    r16 = ais_call(D, nodes, B, shape=16, eval_mode=True)
    eps0, noise_p, noise_e = noise_of(D, B)
    ot = otgt.ManyWell(D)
    ohmc = oais.HMC(M, D, nf.log_prob, ot.log_prob, alpha=2.0, p_target=False, epsilon=0.12, L=L, eval_mode=True)
    oa = oais.AIS(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, ot.log_prob, ohmc, False, 2.0, M)
    opt, olw, _ = oa.sample_and_log_weights(eps0, noise_p, noise_e)
    assert not torch.equal(r4["log_q"], r16["log_q"]), "both runs used the same kernel"
    for tag, x, lw, lq, gq in (("oracle", opt.x.detach(), olw.detach(), opt.log_q.detach(), opt.grad_log_q.detach()),
                               ("16-chain tiles", r16["x"], r16["log_w"], r16["log_q"], r16["grad_log_q"])):
        scale = max(1.0, float(x.abs().max()))
        err = (r4["x"] - x).abs().max(1).values / scale
        print(f"{case_key(D, nodes, B)} vs {tag}: x err {float(err.max()):.2e}  log_w err {max_rel_err(r4['log_w'], lw):.2e}  "
              f"log_q err {max_rel_err(r4['log_q'], lq):.2e}  grad err {max_rel_err(r4['grad_log_q'], gq):.2e}")
        # the acceptance rule of tests/test_gpu_hmc_shapes.py: 1e-4 of the state scale; one chain may differ through an accept
        # decision within rounding of its threshold (it then differs as a whole and is left out of the other comparisons)
        flipped = err > 1e-4
        assert int(flipped.sum()) <= 1, f"{tag}: {int(flipped.sum())} chains differ (max err {float(err.max()):.2e})"
        ok = ~flipped
        assert close(r4["log_w"][ok], lw[ok], RTOL), f"{tag}: log_w err {max_rel_err(r4['log_w'][ok], lw[ok]):.2e}"
        assert close(r4["log_q"][ok], lq[ok], RTOL), f"{tag}: log_q err {max_rel_err(r4['log_q'][ok], lq[ok]):.2e}"
        assert close(r4["grad_log_q"][ok], gq[ok], 5e-4), f"{tag}: grad err {max_rel_err(r4['grad_log_q'][ok], gq[ok]):.2e}"


@pytest.mark.parametrize("D,nodes,B", CASES)
def test_ten_repeated_launches_are_bitwise_equal(tuned, D, nodes, B):
    first = tuned[(D, nodes, B)]
    for rep in range(10):
        again = ais_call(D, nodes, B)
        for name, v in first.items():
            assert torch.equal(v, again[name]), f"launch {rep + 1}: {name} differs"


def test_fast_mode_runs_on_the_same_stages_and_matches_its_emulation():
    """The bf16 W x W stage (r4f_dense_wide_bf16) takes the same hand-over: log q and d log q / dx of the returned points against
    the float64 emulation of tests/test_gpu_fast_mode.py (bf16-rounded W2 and inputs of that Linear) at its bound."""
    import copy
    D, nodes, B = 32, 10, 7
    nf, _ = flows_of(D, nodes)

    class Bf16Linear(torch.nn.Module):
        def __init__(self, lin):
            super().__init__()
            self.w = lin.weight.detach().float().bfloat16().double()
            self.b = lin.bias.detach().double()

        def forward(self, x):
            return x.float().bfloat16().double() @ self.w.t() + self.b

    em = copy.deepcopy(nf).double()
    for f in em.flows:
        if isinstance(f, oflow.AffineCouplingBlock):
            net = f.flows[1].param_map.net
            net[2] = Bf16Linear(net[2])
    rf, rf2 = ais_call(D, nodes, B, fast=True), ais_call(D, nodes, B, fast=True)
    r32 = ais_call(D, nodes, B)
    assert all(torch.equal(rf[k], rf2[k]) for k in rf)
    assert not torch.equal(rf["log_q"], r32["log_q"])
    xg = rf["x"].double().requires_grad_(True)
    lq_e = em.log_prob(xg)
    (g_e,) = torch.autograd.grad(lq_e.sum(), xg)
    dev_em = float((rf["log_q"].double() - lq_e.detach()).abs().max())
    rel = (rf["grad_log_q"].double() - g_e).norm(dim=1) / g_e.norm(dim=1)
    print(f"fast mode vs emulation: log q {dev_em:.2e}  grad median {float(rel.median()):.2e} max {float(rel.max()):.2e}")
    assert dev_em <= 2e-3, f"4-chain fast mode vs its emulation: {dev_em:.2e}"
    assert float(rel.median()) <= 2e-3 and float(rel.max()) <= 5e-2, f"grad vs emulation: {float(rel.max()):.2e}"
