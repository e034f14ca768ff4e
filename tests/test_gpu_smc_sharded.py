"""SMC mode over sharded chains on the GPU (parallel.ShardedAnnealedImportanceSampler(..., resample_across_ranks=True);
include/fabhip.h: fabhip_smc_shard_pack / fabhip_smc_shard_resample) against the single-device SMC call and against its
specification (tests/smc_shard_spec.py).

The inputs are those of tests/test_gpu_smc.py (benign regime); every (inputs, tau) pair used here with the mid threshold is
shown not to be a coin flip by the CPU spec alone in tests/test_smc_shard_spec.py::test_sharded_gpu_thresholds_are_not_coin_flips
(step-size tuning on) and tests/test_gpu_smc.py::test_thresholds_are_not_coin_flips (tuning frozen)."""
import ctypes
import datetime
import os
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import smc_shard_spec

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _lib, _ops, parallel                                   # noqa: E402
from oracle import ais as oais                                                   # noqa: E402
from test_gpu_sharded import _free_port                                          # noqa: E402
from test_gpu_smc import D, DEV, M, TAU_MID, check_decision, inputs, samplers    # noqa: E402

TOTAL = 256
KILL = (235,)                    # a row of the LAST shard for 2 and for 4 ranks


def _shards(total, world, tau, tuning, eps0, na, nb):
    b = total // world
    ranks = [parallel.HipShardBackend(samplers(tau=tau, eval_mode=not tuning)[4]) for _ in range(world)]
    sts = []
    for r, be in enumerate(ranks):
        sl = slice(r * b, (r + 1) * b)
        sts.append(be.begin(b, eps0[sl], na[:, :, sl].contiguous(), nb[:, :, sl].contiguous()))
    return b, ranks, sts


def _emulated_run(world, shape, tau, kill, tuning):
    """One device holding all chains against `world` emulated shards stepped through the backend's methods (the gathered
    buffers concatenated in rank order): everything bit for bit."""
    total = TOTAL
    eps0, na, nb, nr = (t.to(DEV) for t in inputs(total, seed=4, kill=kill))
    with _ops.option(_ops.OPT_TILE_SHAPE, shape):
        _, _, _, op1, ais1 = samplers(tau=tau, eval_mode=not tuning)
        pt, log_w, n_valid, _, _, _ = ais1.run(total, eps0, na, nb, noise_r=nr, trace=True)
        resampled1, ess1, anc1, pre1 = ais1.last_smc
        n0, n1 = (int(v) for v in n_valid.tolist())
        assert n0 == total - len(kill) and n1 == n0
        b, ranks, sts = _shards(total, world, tau, tuning, eps0, na, nb)
        counts = [int(st["n_valid"][0]) for st in sts]
        assert counts == [b] * (world - 1) + [b - len(kill)]
        fired = 0
        for j in range(1, M + 1):
            gathered = torch.cat([be.pack(st) for be, st in zip(ranks, sts)])
            assert gathered.shape == (world * (b + 1), 3 * D + 4)
            for r, (be, st) in enumerate(zip(ranks, sts)):
                keys = ("x", "lq", "lp", "gq", "gp", "log_w")
                tails = [st[k][counts[r]:].clone() for k in keys]
                flag, ess, anc, pre = be.resample(st, j, gathered, world, r, nr[j - 1:j], trace=True)
                for k, t in zip(keys, tails):
                    assert torch.equal(st[k][counts[r]:], t), f"transition {j}, rank {r}: {k} rows beyond n_r changed"
                tag = f"transition {j}, rank {r}"
                assert int(flag) == int(resampled1[j - 1]), f"{tag}: decision"
                assert torch.equal(ess[0], ess1[j - 1]), f"{tag}: ess {float(ess)} vs {float(ess1[j - 1])}"
                assert torch.equal(anc[:n0], anc1[j - 1][:n0]), f"{tag}: ancestors"
                assert torch.equal(pre[:n0], pre1[j - 1][:n0]), f"{tag}: log_w_pre"
                d = check_decision(pre, n0, tau, nr[j - 1], anc, flag[0], ess[0], tag)
            fired += d.resampled
            if tuning:
                slabs = torch.cat([be.step(st, j).clone() for be, st in zip(ranks, sts)])
                for be, st in zip(ranks, sts):
                    be.adapt(st, j, slabs, world)
            else:
                for be, st in zip(ranks, sts):
                    assert be.step(st, j, tune=False) is None
        outs = [be.finish(st) for be, st in zip(ranks, sts)]
    assert fired == M if tau > 1 else 0 < fired < M
    assert [o[0].x.shape[0] for o in outs] == counts
    cat = lambda f: torch.cat([f(o) for o in outs])                                # noqa: E731
    assert torch.equal(cat(lambda o: o[0].x), pt.x[:n1]) and torch.equal(cat(lambda o: o[1]), log_w[:n1])
    assert torch.equal(cat(lambda o: o[0].log_q), pt.log_q[:n1]) and torch.equal(cat(lambda o: o[0].log_p), pt.log_p[:n1])
    assert torch.equal(cat(lambda o: o[0].grad_log_q), pt.grad_log_q[:n1])
    assert torch.equal(cat(lambda o: o[0].grad_log_p), pt.grad_log_p[:n1])
    for be in ranks:
        assert torch.equal(be.op.epsilons, op1.epsilons) and torch.equal(be.op.common_epsilon, op1.common_epsilon)
    if tuning:
        assert not torch.equal(op1.epsilons, samplers()[3].epsilons), "test set-up: the step sizes must have adapted"


@pytest.mark.parametrize("tau", [1.5, TAU_MID])
@pytest.mark.parametrize("shape", [4, 8, 16])
@pytest.mark.parametrize("world", [2, 4])
def test_emulated_shards_reproduce_the_single_device_smc_run_bit_for_bit(world, shape, tau):
    _emulated_run(world, shape, tau, (), tuning=True)


@pytest.mark.parametrize("tau", [1.5, TAU_MID])
@pytest.mark.parametrize("shape", [4, 8, 16])
@pytest.mark.parametrize("world", [2, 4])
def test_emulated_shards_with_a_chain_dropped_in_the_last_shard_reproduce_the_single_device_smc_run(world, shape, tau):
    _emulated_run(world, shape, tau, KILL, tuning=True)


@pytest.mark.parametrize("world,shape", [(2, 8), (4, 4)])
def test_emulated_shards_with_tuning_frozen_step_without_slabs(world, shape):
    _emulated_run(world, shape, TAU_MID, (), tuning=False)


# ---- the two ops in isolation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_grad", [True, False])
@pytest.mark.parametrize("dim", [32, 6])                 # 16-byte rows / the scalar form (3 D + 4 is no multiple of 4 floats)
def test_pack_and_resample_on_hand_built_shards_follow_the_spec(dim, with_grad):
    R, b = 4, 16
    counts = [16, 9, 0, 16]                              # n_r < b on a middle rank, one empty rank
    g = torch.Generator().manual_seed(3)
    r = lambda *sh: torch.randn(*sh, generator=g)        # noqa: E731
    host = [dict(x=r(b, dim), lq=r(b), lp=r(b), gq=r(b, dim) if with_grad else None, gp=r(b, dim) if with_grad else None,
                 log_w=2.0 * r(b)) for _ in range(R)]
    u = torch.rand(1, generator=g, dtype=torch.float64)
    ops = _ops.load()
    to = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    points = [oais.Point(h["x"], h["lq"], h["lp"], h["gq"], h["gp"]) for h in host]
    log_ws = [h["log_w"] for h in host]
    for tau in (1.5, 0.0):
        dev = [{k: to(v) for k, v in h.items()} for h in host]
        nv = [torch.tensor([n, 0], dtype=torch.int32, device=DEV) for n in counts]
        sends = [ops.smc_shard_pack(s["x"], s["lq"], s["lp"], s["gq"], s["gp"], s["log_w"], n) for s, n in zip(dev, nv)]
        for rk, send in enumerate(sends):
            want = smc_shard_spec.pack_state(points[rk], log_ws[rk], counts[rk])
            got = send.cpu()
            assert got.shape == (b + 1, 3 * dim + 4)
            cols = list(range(3 * dim + 4)) if with_grad else list(range(dim)) + list(range(3 * dim, 3 * dim + 4))
            assert torch.equal(got[:b][:, cols], want[:b][:, cols]), f"rank {rk}: packed rows"
            assert torch.equal(got[b].view(torch.int32), want[b].view(torch.int32)), f"rank {rk}: trailer"
        gathered = torch.cat(sends).reshape(R, b + 1, 3 * dim + 4)
        want_p, want_w, d = smc_shard_spec.resample_step(points, log_ws, counts, tau, float(u))
        assert d.resampled == (tau > 1)
        n0 = sum(counts)
        for rk, (s, n) in enumerate(zip(dev, nv)):
            flag, ess, anc, pre = ops.smc_shard_resample(gathered, R, rk, tau, u.to(DEV), s["x"], s["lq"], s["lp"], s["gq"], s["gp"],
                                                         s["log_w"], n, True)
            assert int(flag) == int(d.resampled) and abs(float(ess) - d.ess) <= 1e-6 * d.ess
            assert anc.shape == (R * b,) and np.array_equal(anc[:n0].cpu().numpy().astype(np.int64), d.ancestors)
            assert torch.equal(anc[n0:].cpu(), torch.arange(n0, R * b, dtype=torch.int32))
            glob_lw = torch.cat([lw[:c] for lw, c in zip(log_ws, counts)])
            assert torch.equal(pre[:n0].cpu(), glob_lw) and bool(torch.isinf(pre[n0:]).all())
            for k, name in (("x", "x"), ("lq", "log_q"), ("lp", "log_p"), ("gq", "grad_log_q"), ("gp", "grad_log_p")):
                if s[k] is not None:
                    assert torch.equal(s[k].cpu(), getattr(want_p[rk], name)), f"tau {tau}, rank {rk}: {name}"
            lw, c = s["log_w"].cpu(), counts[rk]
            assert torch.equal(lw[c:], log_ws[rk][c:])
            if tau > 1 and c:     # the common log-weight: the decision kernel's float32 of a float64 log, as in tests/test_gpu_smc.py
                assert bool((lw[:c] == lw[0]).all()) and abs(float(lw[0]) - d.log_w_common) <= 1e-6 * max(1.0, abs(d.log_w_common))
            else:
                assert torch.equal(lw, log_ws[rk])
            assert torch.equal(n.cpu(), torch.tensor([counts[rk], 0], dtype=torch.int32))


def test_c_abi_refusals():
    lib = _lib.load()
    R, b, dim = 2, 16, 8
    f32 = dict(dtype=torch.float32, device=DEV)
    x, lq, lp, lw = torch.zeros(b, dim, **f32), torch.zeros(b, **f32), torch.zeros(b, **f32), torch.zeros(b, **f32)
    nv = torch.tensor([b, 0], dtype=torch.int32, device=DEV)
    u = torch.zeros(1, dtype=torch.float64, device=DEV)
    gathered = torch.zeros(64 + 1, b + 1, 3 * dim + 4, **f32)
    nbytes = lib.fabhip_smc_shard_workspace_bytes(R, b)
    assert nbytes > 0 and lib.fabhip_smc_shard_workspace_bytes(65, b) == 0 and lib.fabhip_smc_shard_workspace_bytes(64, b) > 0
    ws = torch.empty(lib.fabhip_smc_shard_workspace_bytes(64, b) + 256, dtype=torch.uint8, device=DEV)
    wsp = ctypes.c_void_p((ws.data_ptr() + 255) & ~255)
    p = _lib.ptr
    pt = _lib.Point(p(x), p(lq), p(lp), None, None)
    call = lambda R_, pt_, nb_: lib.fabhip_smc_shard_resample(p(gathered), R_, 0, b, dim, 1.5, p(u), ctypes.byref(pt_), p(lw),      # noqa: E731
                                                              p(nv), None, None, None, None, wsp, nb_, _lib.stream_ptr())
    assert call(65, pt, 1 << 30) == -2                                           # FABHIP_ENOTSUP: more than 64 ranks
    assert call(R, pt, nbytes - 1) == -4                                         # FABHIP_ENOSPC
    assert call(R, _lib.Point(None, p(lq), p(lp), None, None), nbytes) == -1     # FABHIP_EINVAL: no state
    assert call(R, _lib.Point(p(x), p(lq), p(lp), p(x), None), nbytes) == -1     # one gradient without the other
    assert lib.fabhip_smc_shard_pack(ctypes.byref(pt), p(lw), None, b, dim, p(gathered), _lib.stream_ptr()) == -1
    assert call(R, pt, nbytes) == 0                                              # and the call the refusals were variations of
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="fabhip"):                            # the op: a gathered buffer of the wrong size
        _ops.load().smc_shard_resample(gathered[:1], R, 0, 1.5, u, x, lq, lp, None, None, lw, nv, False)
    with pytest.raises(RuntimeError, match="fabhip"):                            # u is validated like noise_r: float64
        _ops.load().smc_shard_resample(gathered[:R], R, 0, 1.5, u.float(), x, lq, lp, None, None, lw, nv, False)


# ---- the sampler -------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, total, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    torch.manual_seed(50 + rank)
    _, _, _, op, ais = samplers(tau=TAU_MID, eval_mode=False)
    sh = parallel.ShardedAnnealedImportanceSampler(ais, resample_across_ranks=True)
    b = total // world
    eps0, na, nb, nr = (t.to(DEV) for t in inputs(total, seed=5))
    sl = slice(rank * b, (rank + 1) * b)
    res = {}
    with _ops.option(_ops.OPT_TILE_SHAPE, 4):
        import warnings
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for it in range(2):                                  # two calls: the adapted step sizes carry over
                x, lw, lq = sh.sample_and_log_weights(total, eps0=eps0[sl], noise_a=na[:, :, sl].contiguous(),
                                                      noise_b=nb[:, :, sl].contiguous(), noise_r=nr if it == 0 else None,
                                                      trace=True)
                res[it] = (x.cpu(), lw.cpu(), sh.last_noise_r.cpu(), [t.cpu() for t in sh.last_smc])
    torch.save({"res": res, "eps": op.epsilons.cpu(), "ceps": op.common_epsilon.cpu(), "n_slab": sh.n_slab_gathers,
                "n_state": sh.n_state_gathers, "n_resampled": int(sh.logging_info["n_resampled"]),
                "ess_min": float(sh.logging_info["ess_min_in_chain"]),
                "warned": sum("Python-stepped loop" in str(w.message) for w in caught)}, out + str(rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_processes_on_one_gpu_reproduce_the_single_process_smc_run(tmp_path):
    """Two real processes (gloo rendezvous, both on the one GPU of the box, payload staged through the host) against the fused
    single-device SMC call.  The first call gets its uniforms from the caller, the second from rank 0's broadcast draw."""
    world, total = 2, TOTAL
    out = str(tmp_path / "g")
    ctx = mp.spawn(_worker, args=(world, _free_port(), total, out), nprocs=world, join=False)
    deadline = time.time() + 300
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail("the two-process run did not finish within its time limit")
    r0, r1 = torch.load(out + "0", weights_only=False), torch.load(out + "1", weights_only=False)
    _, _, _, op, ais = samplers(tau=TAU_MID, eval_mode=False)
    eps0, na, nb, nr = (t.to(DEV) for t in inputs(total, seed=5))
    assert torch.equal(r0["res"][0][2], nr.cpu()) and torch.equal(r0["res"][1][2], r1["res"][1][2])
    assert not torch.equal(r0["res"][1][2], nr.cpu())
    with _ops.option(_ops.OPT_TILE_SHAPE, 4):
        for it in range(2):
            pt, lw = ais.sample_and_log_weights(total, eps0=eps0, noise_a=na, noise_b=nb, noise_r=r0["res"][it][2].to(DEV))
            resampled, ess = ais.last_smc[0].cpu(), ais.last_smc[1].cpu()
            for r in (r0, r1):
                assert torch.equal(r["res"][it][0], pt.x.cpu()) and torch.equal(r["res"][it][1], lw.cpu())
                assert torch.equal(r["res"][it][3][0], resampled) and torch.equal(r["res"][it][3][1], ess)
                assert r["res"][it][3][2].shape == (M, total)
    info = ais.get_logging_info()
    for r in (r0, r1):
        assert torch.equal(r["eps"], op.epsilons.cpu()) and torch.equal(r["ceps"], op.common_epsilon.cpu())
        assert r["n_state"] == M and r["n_slab"] == M and r["warned"] == 1
        assert r["n_resampled"] == info["n_resampled"] and abs(r["ess_min"] - info["ess_min_in_chain"]) <= 1e-6


def test_one_rank_group_with_the_opt_in_is_the_fused_smc_call_and_a_missing_threshold_changes_nothing():
    B = TOTAL
    eps0, na, nb, nr = (t.to(DEV) for t in inputs(B, seed=4))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1, timeout=datetime.timedelta(seconds=120))
    try:
        _, _, _, op1, ais1 = samplers(tau=TAU_MID, eval_mode=False)
        _, _, _, op2, ais2 = samplers(tau=TAU_MID, eval_mode=False)
        pt, lw = ais1.sample_and_log_weights(B, eps0=eps0, noise_a=na, noise_b=nb, noise_r=nr)
        sh = parallel.ShardedAnnealedImportanceSampler(ais2, resample_across_ranks=True)
        x, lw2, lq = sh.sample_and_log_weights(B, eps0=eps0, noise_a=na, noise_b=nb, noise_r=nr)
        assert torch.equal(x, pt.x) and torch.equal(lw2, lw) and torch.equal(lq, pt.log_q)
        assert torch.equal(op2.epsilons, op1.epsilons) and torch.equal(op2.common_epsilon, op1.common_epsilon)
        assert sh.n_state_gathers == 0 and sh.n_slab_gathers == 0
        assert torch.equal(sh.last_smc[0], ais1.last_smc[0]) and torch.equal(sh.last_smc[1], ais1.last_smc[1])
        assert int(sh.logging_info["n_resampled"]) == ais1.get_logging_info()["n_resampled"] > 0
        # the mode argument on, resample_threshold = None: today's sharded run, bit for bit
        outs = []
        for kw in ({}, {"resample_across_ranks": True}):
            _, _, _, op, ais = samplers(tau=None, eval_mode=False)
            s = parallel.ShardedAnnealedImportanceSampler(ais, **kw)
            xs, lws, lqs = s.sample_and_log_weights(B, eps0=eps0, noise_a=na, noise_b=nb)
            outs.append((xs, lws, lqs, op.epsilons.clone(), op.common_epsilon.clone()))
            assert s.n_state_gathers == 0 and s.last_smc is None and "n_resampled" not in s.logging_info
        assert all(torch.equal(u, v) for u, v in zip(*outs))
        # the default still refuses; Metropolis with the mode on is refused by name
        with pytest.raises(_ops.FabhipError, match="resample_threshold"):
            parallel.ShardedAnnealedImportanceSampler(ais2).sample_and_log_weights(B)
        _, _, _, _, aism = samplers(hmc=False, tau=TAU_MID)
        with pytest.raises(_ops.FabhipError, match="Metropolis"):
            parallel.ShardedAnnealedImportanceSampler(aism, resample_across_ranks=True).sample_and_log_weights(B)
    finally:
        dist.destroy_process_group()
