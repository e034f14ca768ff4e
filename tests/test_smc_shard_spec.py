"""SMC mode over sharded chains on the CPU: the specification (tests/smc_shard_spec.py) against the single-device one
(tests/smc_spec.py), and the host logic of `parallel.ShardedAnnealedImportanceSampler(..., resample_across_ranks=True)` in a
two-process gloo run with an oracle-backed stand-in backend (the pattern of tests/test_parallel_gloo.py)."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import ROOT, seeded_oracle_flow

import smc_shard_spec
import smc_spec
from fab_torch_amd import _ops, parallel
from oracle import ais as oais
from oracle import targets as otgt
from test_parallel_gloo import _OracleShardBackend, _free_port, _sharded_noise


# ---- 1. the sharded definition is the single-device one on the concatenation -----------------------------------------------------
def _random_shards(g, R, b, D, counts, spread, with_grad=True):
    points, log_ws = [], []
    for _ in range(R):
        r = lambda *sh: torch.randn(*sh, generator=g)                                            # noqa: E731
        points.append(oais.Point(r(b, D), r(b), r(b), r(b, D) if with_grad else None, r(b, D) if with_grad else None))
        log_ws.append(spread * r(b))
    return points, log_ws


@pytest.mark.parametrize("tau", [1.5, 0.5, 0.0, -1.0])
@pytest.mark.parametrize("counts", [(8, 8, 8), (8, 0, 5), (0, 3, 8, 8), (7, 8), (1,), (5, 8, 0)])
@pytest.mark.parametrize("with_grad", [True, False])
def test_sharded_step_equals_the_single_device_step_on_the_concatenation(counts, tau, with_grad):
    b, D, R = 8, 5, len(counts)
    g = torch.Generator().manual_seed(17 * R + sum(counts))
    points, log_ws = _random_shards(g, R, b, D, counts, 3.0, with_grad)
    if counts[-1] > 1:
        log_ws[-1][0] = float("nan")                                  # a live row without weight
    u = float(torch.rand(1, generator=g, dtype=torch.float64))
    cat = lambda name: None if getattr(points[0], name) is None else torch.cat(                  # noqa: E731
        [getattr(p, name)[:n] for p, n in zip(points, counts)])
    glob = oais.Point(cat("x"), cat("log_q"), cat("log_p"), cat("grad_log_q"), cat("grad_log_p"))
    glob_lw = torch.cat([lw[:n] for lw, n in zip(log_ws, counts)])
    want_pt, want_lw, want_d = smc_spec.resample_step(glob, glob_lw, tau, u)
    out_p, out_w, d = smc_shard_spec.resample_step(points, log_ws, counts, tau, u)
    assert d.resampled == want_d.resampled and d.ess == want_d.ess and np.array_equal(d.ancestors, want_d.ancestors)
    assert d.resampled == (tau > 1.0) or 0.0 < tau <= 1.0           # tau > 1: always, tau <= 0: never
    off = smc_shard_spec.offsets(counts)
    eq = lambda a, c: torch.equal(a.nan_to_num(nan=7.0), c.nan_to_num(nan=7.0))                   # noqa: E731
    for r, n in enumerate(counts):
        sl = slice(off[r], off[r] + n)
        for name in ("x", "log_q", "log_p", "grad_log_q", "grad_log_p"):
            got, was = getattr(out_p[r], name), getattr(points[r], name)
            if got is None:
                assert not with_grad and name.startswith("grad")
                continue
            assert torch.equal(got[:n], getattr(want_pt, name)[sl]), f"rank {r}: {name}"
            assert torch.equal(got[n:], was[n:]), f"rank {r}: {name} rows beyond n_r must stay"
        assert eq(out_w[r][:n], want_lw[sl]) and eq(out_w[r][n:], log_ws[r][n:])
    # the wire format round-trips, and the step through it gives the same rows
    gathered = torch.cat([smc_shard_spec.pack_state(p, lw, n) for p, lw, n in zip(points, log_ws, counts)])
    assert gathered.shape == (R * (b + 1), 3 * D + 4)
    for r in range(R):
        pt, lw, d2, cn = smc_shard_spec.resample_gathered(gathered, R, r, with_grad, tau, u)
        assert cn == list(counts) and d2.resampled == d.resampled
        assert torch.equal(pt.x, out_p[r].x) and torch.equal(pt.log_q, out_p[r].log_q) and eq(lw, out_w[r])
        if with_grad:
            assert torch.equal(pt.grad_log_p, out_p[r].grad_log_p)


# ---- 2. the host loop over two gloo ranks --------------------------------------------------------------------------------------
TAU_GLOO = 0.5


class _OracleSmcShardBackend(_OracleShardBackend):
    """_OracleShardBackend + the two methods of the SMC mode over ranks, through the specification's wire format."""
    device = "cpu"

    def __init__(self, tau, tuning=True):
        super().__init__()
        self.tuning = tuning
        self.ais = types.SimpleNamespace(resample_threshold=tau, last_smc=None)
        self.decisions = []

    def step(self, st, j, tune=True):
        slab = super().step(st, j)
        return slab if tune else None

    def pack(self, st):
        return smc_shard_spec.pack_state(st["pt"], st["lw"].float(), st["b"])

    def resample(self, st, j, gathered, world, rank, u_j, trace=False):
        assert u_j.dtype == torch.float64 and u_j.shape == (1,)
        pt, lw, d, counts = smc_shard_spec.resample_gathered(gathered, world, rank, True, self.ais.resample_threshold, float(u_j))
        lw_pre = torch.cat([g[:n] for g, n in zip(smc_shard_spec.unpack_state(gathered, world, True)[1], counts)])
        st["pt"], st["lw"] = pt, lw
        self.decisions.append((d.resampled, d.ess, d.ancestors.copy()))
        e = torch.empty(0)
        return (torch.tensor([int(d.resampled)], dtype=torch.int32), torch.tensor([d.ess], dtype=torch.float32),
                torch.as_tensor(d.ancestors, dtype=torch.int32) if trace else e.int(), lw_pre if trace else e)


def _worker_smc(rank, world, port, total, out, tuning, explicit_noise):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    torch.manual_seed(1000 + rank)                           # the ranks' own generators differ: a shared draw must be broadcast
    be = _OracleSmcShardBackend(TAU_GLOO, tuning)
    sh = parallel.ShardedAnnealedImportanceSampler(backend=be, resample_across_ranks=True)
    b = total // world
    eps0, na, nb = _sharded_noise(total, be.D, be.M)
    nr = _gloo_noise_r(be.M) if explicit_noise else None
    sl = slice(rank * b, (rank + 1) * b)
    x, lw, lq = sh.sample_and_log_weights(total, eps0=eps0[sl], noise_a=na[:, :, sl].contiguous(),
                                          noise_b=nb[:, :, sl].contiguous(), noise_r=nr, trace=True)
    torch.save({"x": x, "lw": lw, "eps": be.hmc.epsilons.clone(), "ceps": be.hmc.common_epsilon.clone(), "ups": [t[0] for t in be.trace],
                "decisions": be.decisions, "n_slab": sh.n_slab_gathers, "n_state": sh.n_state_gathers, "noise_r": sh.last_noise_r,
                "last_smc": sh.last_smc, "n_resampled": int(sh.logging_info["n_resampled"]),
                "ess_min": float(sh.logging_info["ess_min_in_chain"])}, out + str(rank))
    dist.barrier()
    dist.destroy_process_group()


def _gloo_noise_r(M):
    return torch.rand(M, dtype=torch.float64, generator=torch.Generator().manual_seed(23))


def _single_device_smc(be, total, noise_r, tuning):
    """smc_spec.SMC holding all chains: the oracle's own HMC (its own step-size rule when tuning is on)."""
    hmc = oais.HMC(be.M, be.D, be.nf.log_prob, be.target.log_prob, alpha=2.0, p_target=False, epsilon=0.25, L=3,
                   eval_mode=not tuning)
    s = smc_spec.SMC(lambda e: tuple(t.detach() for t in be.nf.sample_eps(e)), be.nf.log_prob, be.target.log_prob, hmc, False, 2.0,
                     be.M, resample_threshold=TAU_GLOO)
    eps0, na, nb = _sharded_noise(total, be.D, be.M)
    pt, lw, _ = s.sample_and_log_weights(eps0, na, nb, noise_r=noise_r)
    return s, hmc, pt, lw


@pytest.mark.parametrize("tuning,explicit_noise", [(True, True), (False, False)], ids=["tuning_on", "tuning_frozen_drawn_uniforms"])
def test_two_rank_smc_run_reproduces_the_single_device_smc_run(tmp_path, tuning, explicit_noise):
    """2 ranks x 32 chains against smc_spec.SMC holding all 64 chains on the same noise rows: identical decisions, ancestors and
    step-size decisions; particles and weights at the tolerances of tests/test_parallel_gloo.py for the oracle's own arithmetic;
    one state gather per transition, one slab gather per transition while tuning is on and none with tuning frozen.  Without
    `noise_r` rank 0's draw reaches both ranks (their generators are seeded differently)."""
    world, total = 2, 64
    out = str(tmp_path / "s")
    mp.spawn(_worker_smc, args=(world, _free_port(), total, out, tuning, explicit_noise), nprocs=world, join=True)
    r0, r1 = torch.load(out + "0", weights_only=False), torch.load(out + "1", weights_only=False)
    torch.set_num_threads(1)
    be = _OracleShardBackend()
    M = be.M
    assert r0["noise_r"].dtype == torch.float64 and r0["noise_r"].shape == (M,) and torch.equal(r0["noise_r"], r1["noise_r"])
    if explicit_noise:
        assert torch.equal(r0["noise_r"], _gloo_noise_r(M))
    assert bool(((r0["noise_r"] >= 0) & (r0["noise_r"] < 1)).all())
    s, hmc, pt, lw = _single_device_smc(be, total, r0["noise_r"], tuning)
    assert any(s.trace.resampled) and not all(s.trace.resampled), "test set-up: both outcomes of the decision must occur"
    assert all(abs(e - TAU_GLOO) >= 1e-2 * TAU_GLOO for e in s.trace.ess), "test set-up: a decision is a coin flip"
    for r in (r0, r1):
        assert [d[0] for d in r["decisions"]] == s.trace.resampled
        for j in range(M):
            assert np.array_equal(r["decisions"][j][2], s.trace.ancestors[j]), f"transition {j + 1}: ancestors"
            assert abs(r["decisions"][j][1] - s.trace.ess[j]) <= 1e-4 * s.trace.ess[j]
        assert r["n_state"] == M and r["n_slab"] == (M if tuning else 0)
        assert torch.equal(r["eps"], hmc.epsilons) and torch.equal(r["ceps"], hmc.common_epsilon)      # the same up / down decisions
        assert len(r["ups"]) == (M if tuning else 0)
        resampled, ess, anc, lw_pre = r["last_smc"]
        assert resampled.tolist() == [int(f) for f in s.trace.resampled] and anc.shape == (M, total) and lw_pre.shape == (M, total)
        assert r["n_resampled"] == sum(s.trace.resampled) and abs(r["ess_min"] - min(s.trace.ess)) <= 1e-4 * min(s.trace.ess)
    assert torch.equal(r0["x"], r1["x"]) and torch.equal(r0["lw"], r1["lw"])
    np.testing.assert_allclose(r0["x"].numpy(), pt.x.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r0["lw"].numpy(), lw.numpy(), rtol=1e-4, atol=1e-4)


# ---- 3. arguments and refusals ---------------------------------------------------------------------------------------------------
def test_argument_checks_and_refusals():
    be = _OracleSmcShardBackend(0.5)
    M = be.M
    sh = parallel.ShardedAnnealedImportanceSampler(backend=be, resample_across_ranks=True)
    eps0, na, nb = _sharded_noise(32, be.D, M)
    with pytest.raises(_ops.FabhipError, match="noise_r"):
        sh.sample_and_log_weights(32, eps0=eps0, noise_a=na, noise_b=nb, noise_r=torch.rand(M))                  # float32
    with pytest.raises(_ops.FabhipError, match="noise_r"):
        sh.sample_and_log_weights(32, eps0=eps0, noise_a=na, noise_b=nb, noise_r=torch.rand(M + 1, dtype=torch.float64))
    # Metropolis with the mode on: refused by name
    bm = _OracleSmcShardBackend(0.5)
    bm.hmc = None
    with pytest.raises(_ops.FabhipError, match="Metropolis"):
        parallel.ShardedAnnealedImportanceSampler(backend=bm, resample_across_ranks=True).sample_and_log_weights(32)
    # noise_r without the mode / without a threshold
    plain = _OracleSmcShardBackend(None)
    with pytest.raises(_ops.FabhipError, match="noise_r"):
        parallel.ShardedAnnealedImportanceSampler(backend=plain, resample_across_ranks=True).sample_and_log_weights(
            32, noise_r=torch.rand(M, dtype=torch.float64))
    # the default still refuses, with the old match, and so does the helper
    for kw in ({}, {"resample_across_ranks": False}):
        with pytest.raises(_ops.FabhipError, match="resample_threshold"):
            parallel.ShardedAnnealedImportanceSampler(backend=_OracleSmcShardBackend(0.5), **kw).sample_and_log_weights(32)
    with pytest.raises(_ops.FabhipError, match="resample_threshold"):
        parallel.refuse_resampling("somebody", 0.5)
    parallel.refuse_resampling("somebody", None)
    sh0 = parallel.ShardedAnnealedImportanceSampler(backend=plain)
    assert sh0.resample_across_ranks is False and sh0.n_state_gathers == 0 and sh0.last_smc is None


# ---- 4. the thresholds of tests/test_gpu_smc_sharded.py are not coin flips ---------------------------------------------------------
# (B, seed, killed rows) of test_gpu_smc.inputs that the GPU tests run with tuning ON and TAU_MID; their tau = 1.5 runs resample
# before every transition whatever the ess (<= 1), the tau = 0 run of the isolated gather never does.
GPU_TAU_MID = 0.05
GPU_MID_CASES = ((256, 4, ()), (256, 4, (235,)), (256, 5, ()))


def _gpu_inputs(B, seed, kill):
    """test_gpu_smc.inputs(B, seed, hmc=True, kill) restated (that module needs the GPU build to import)."""
    D, M = 32, 4
    g = torch.Generator().manual_seed(100 + seed)
    eps0 = torch.randn(B, D, generator=g)
    for r in kill:
        eps0[r] = float("inf")
    na = torch.randn(M, 1, B, D, generator=g)
    nb = torch.empty(M, 1, B).exponential_(1.0, generator=g)
    nr = torch.rand(M, generator=g, dtype=torch.float64)
    return eps0, na, nb, nr


def test_sharded_gpu_thresholds_are_not_coin_flips():
    """The CPU spec alone, step-size tuning ON as in the GPU tests: every ess is at least a relative 1e-2 away from TAU_MID (the
    device-side tests assert 1e-3 on the device's own weights) and both outcomes of the decision occur."""
    D, K, NODES, M, L, STEP = 32, 3, 10, 4, 3, 0.05
    for B, seed, kill in GPU_MID_CASES:
        eps0, na, nb, nr = _gpu_inputs(B, seed, kill)
        nf = seeded_oracle_flow(D, K, NODES, 7, std=0.01)
        ot = otgt.ManyWell(D)
        hmc = oais.HMC(M, D, nf.log_prob, ot.log_prob, alpha=2.0, p_target=False, epsilon=STEP, L=L, eval_mode=False)
        s = smc_spec.SMC(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, ot.log_prob, hmc, False, 2.0, M,
                         resample_threshold=GPU_TAU_MID)
        s.sample_and_log_weights(eps0, na, nb, noise_r=nr)
        print(B, seed, kill, [round(e, 4) for e in s.trace.ess], s.trace.resampled)
        assert all(abs(e - GPU_TAU_MID) >= 1e-2 * GPU_TAU_MID for e in s.trace.ess)
        assert any(s.trace.resampled) and not all(s.trace.resampled)
        assert all(0.0 < e <= 1.0 for e in s.trace.ess)                # tau = 1.5 always fires, tau = 0 never
