"""GPU tests of the training half of a FAB iteration as built in round 6: the replay-buffer minibatch step as ONE op
(`fabhip::buffer_train_step`: fab/train_with_prioritised_buffer.py:158-185 + prioritised_replay_buffer.py:117-131), the buffer's
`add` and its row selection as one op each, the tape forward on 8-chain tiles and the tile GEMM of the parameter gradients
against the kernels they replace."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _flow(D, K, nodes, dev, act_norm=False, seed=0):
    import fab_torch_amd as fa
    torch.manual_seed(seed)
    flow = fa.make_wrapped_normflow_realnvp(D, K, nodes, act_norm=act_norm).to(dev)
    with torch.no_grad():
        for l1, l2, l3, aff in flow._layers():
            l3.weight.add_(0.01 * torch.randn_like(l3.weight))
            l3.bias.add_(0.01 * torch.randn_like(l3.bias))
    return flow


@pytest.mark.parametrize("D,K,nodes,B,an", [(32, 4, 10, 2048, False), (6, 8, 40, 1000, False), (2, 4, 40, 77, False),
                                            (60, 3, 4, 333, False), (33, 2, 8, 130, True), (12, 3, 20, 4096, False),
                                            (32, 2, 6, 5, False)])
def test_tile_gemm_parameter_gradients_equal_the_block_kernel(D, K, nodes, B, an):
    """k_pgrad_tiles (default) against the round-1 64 x 64 block kernel (FABHIP_PGRAD=0) on the same tape: every parameter
    tensor to 2e-5 of the image's largest entry (two fp32 summation orders of B terms), bitwise reproducible."""
    from fab_torch_amd import _ops
    dev = torch.device("cuda", 0)
    flow = _flow(D, K, nodes, dev, an)
    x = torch.randn(B, D, device=dev)
    coef = torch.randn(B, device=dev) / B
    lq, tape = flow.log_prob_with_tape(x)
    assert bool(torch.isfinite(lq).all())
    res = {}
    for mode in (0, 1):
        with _ops.option(_ops.OPT_PGRAD, mode):
            res[mode] = [flow.param_grad_flat(tape, coef).clone() for _ in range(3)]
    a, b = res[0][0], res[1][0]
    assert all(torch.equal(b, r) for r in res[1])
    assert bool(torch.isfinite(b).all())
    assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-7


@pytest.mark.parametrize("D,K,nodes,B", [(32, 3, 8, 100), (32, 10, 10, 515), (6, 8, 40, 1000), (12, 3, 20, 37), (32, 2, 10, 8)])
def test_eight_chain_tape_forward_matches_the_sixteen_chain_kernel(D, K, nodes, B):
    """fabhip_flow_log_prob_tape on 8-chain stream tiles (default where the flow has that image) against the 16-chain kernel
    (FABHIP_TAPE_TILES=16): log q to 1e-5; the parameter gradients of each tape against the float64 oracle are covered by
    test_gpu_parity.py::test_flow_parameter_gradients_vs_oracle_autograd (whichever kernel the shape selects); here the two
    kernels' gradients agree wherever no hidden unit sits within rounding distance of its ReLU kink (rows whose ReLU decisions
    agree in both tapes)."""
    from fab_torch_amd import _ops
    dev = torch.device("cuda", 0)
    ops = _ops.load()
    flow = _flow(D, K, nodes, dev)
    x = torch.randn(B, D, device=dev)
    lay = [int(v) for v in ops.flow_tape_layout(D, K, D * nodes, B)]
    Bp, wz, w1, wh, wp, we, wb, oZA, oGZ, oZ1, oH1, oH2, oDP, oE2, oE1, stride, oTB, total = lay
    out = {}
    for mode in (16, 0):
        with _ops.option(_ops.OPT_TAPE_TILES, mode):
            lq, tape, gx = flow.log_prob_with_tape(x, want_grad_x=True)
            lq2, tape2, _ = flow.log_prob_with_tape(x, want_grad_x=True)
            assert torch.equal(lq, lq2)
            out[mode] = (lq.clone(), gx.clone(), tape[0][:total].clone())
    a, b = out[16], out[0]
    assert float(((a[0] - b[0]).abs() / a[0].abs().clamp(min=1.0)).max()) < 1e-5
    # rows with identical ReLU decisions in every layer (H1 / H2 > 0 patterns): their tape rows and input gradients agree
    same = torch.ones(B, dtype=torch.bool, device=dev)
    for k in range(K):
        for o in (oH1, oH2):
            ha = a[2][k * stride + o: k * stride + o + Bp * wh].view(Bp, wh)[:B, :D * nodes]
            hb = b[2][k * stride + o: k * stride + o + Bp * wh].view(Bp, wh)[:B, :D * nodes]
            same &= ((ha > 0) == (hb > 0)).all(dim=1)
    assert int(same.sum()) >= (B * 3) // 4
    ga, gb = a[1][same], b[1][same]
    assert float((ga - gb).abs().max()) <= 2e-4 * float(ga.abs().max()) + 1e-6
    for k in range(K):
        for o, w in ((oZA, wz), (oGZ, wz), (oH1, wh), (oH2, wh), (oDP, wp), (oE2, we), (oE1, we)):
            ta = a[2][k * stride + o: k * stride + o + Bp * w].view(Bp, w)[:B][same]
            tb = b[2][k * stride + o: k * stride + o + Bp * w].view(Bp, w)[:B][same]
            assert float((ta - tb).abs().max()) <= 2e-4 * float(ta.abs().max()) + 1e-6, (k, o)


def test_tape_forward_reads_the_minibatch_in_place_from_the_buffer():
    """fabhip_flow_log_prob_tape_rows: batch row g = row rows[g] of the buffer - bit-identical to gathering first, on both tile
    shapes (through the one-op step's building blocks: the C ABI driven with ctypes)."""
    import ctypes as C
    from fab_torch_amd import _lib, _ops
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lib.fabhip_flow_log_prob_tape_rows.argtypes = [C.POINTER(_lib.Flow), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                   C.c_void_p, C.c_size_t, C.c_void_p]
    lib.fabhip_flow_tape_bytes.restype = C.c_size_t
    lib.fabhip_flow_tape_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    for (D, K, nodes) in ((32, 3, 10), (6, 3, 8)):
        flow = _flow(D, K, nodes, dev)
        packed, _, _, W = flow.native(need_inverse=False)
        bufx = torch.randn(5000, D, device=dev)
        rows = torch.randperm(5000, device=dev)[:300].contiguous()
        nb = lib.fabhip_flow_tape_bytes(D, K, W, 300)
        f = _lib.Flow(D, K, W, _lib.ptr(packed))
        for mode in (0, 16):
            with _ops.option(_ops.OPT_TAPE_TILES, mode):
                lq_a, tape_a = flow.log_prob_with_tape(bufx[rows])
                lq_b = torch.empty(300, device=dev)
                tape_b = torch.empty(nb // 4 + 64, device=dev)
                _lib.check(lib.fabhip_flow_log_prob_tape_rows(C.byref(f), _lib.ptr(bufx), _lib.ptr(rows), _lib.ptr(lq_b), None, 300,
                                                              _lib.ptr(tape_b), nb, _lib.stream_ptr()), "tape_rows")
                torch.cuda.synchronize()
                assert torch.equal(lq_a, lq_b)


def test_buffer_add_and_sample_ops_match_the_tensor_expressions():
    """fabhip::buffer_add = the ring write of prioritised_replay_buffer.py:71-85 (incl. the wrap); fabhip_buffer_sample with
    given uniforms = top-k of logit + Gumbel(u) as a set, ordered by the second set of uniforms."""
    import ctypes as C
    from fab_torch_amd import _lib, _ops
    dev = torch.device("cuda", 0)
    ops = _ops.load()
    L, D = 1000, 7
    bx, blw, blq = torch.zeros(L, D, device=dev), torch.zeros(L, device=dev), torch.zeros(L, device=dev)
    rx, rlw, rlq = bx.clone(), blw.clone(), blq.clone()
    start = 0
    for n in (300, 300, 300, 300, 17):
        x, lw, lq = torch.randn(n, D, device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev)
        ops.buffer_add(x, lw, lq, start, bx, blw, blq)
        idx = (torch.arange(n, device=dev) + start) % L
        rx[idx], rlw[idx], rlq[idx] = x, lw, lq
        start = (start + n) % L
        assert torch.equal(bx, rx) and torch.equal(blw, rlw) and torch.equal(blq, rlq)
    lib = _lib.load()
    lib.fabhip_buffer_sample_workspace_bytes.restype = C.c_size_t
    lib.fabhip_buffer_sample_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
    lib.fabhip_buffer_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]
    for n, k in ((100000, 4096), (512000, 16384), (300, 300), (50, 1), (200000, 50000)):
        g = torch.Generator(device=dev).manual_seed(n)
        logw = torch.randn(n, device=dev, generator=g) * 3
        logw[::7] = -float("inf")
        u = torch.rand(n, device=dev, generator=g)
        r = torch.rand(4, device=dev, generator=g)
        nb = lib.fabhip_buffer_sample_workspace_bytes(n, k)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
        wsp = (ws.data_ptr() + 255) & ~255
        out = torch.empty(k, dtype=torch.int64, device=dev)
        _lib.check(lib.fabhip_buffer_sample(_lib.ptr(logw), _lib.ptr(u), _lib.ptr(r), n, k, _lib.ptr(out), C.c_void_p(wsp), nb,
                                            _lib.stream_ptr()), "buffer_sample")
        keys = -torch.log(-torch.log(u.clamp(min=torch.finfo(torch.float32).tiny))) + logw
        if k < n:
            kth = torch.topk(keys, k).values.min()
            assert bool((keys[out] >= kth).all())
        assert out.unique().numel() == k
        # the order: a bijection of the selection (keyed by r), another key = another order, the same key = the same order
        sel_sorted = torch.sort(out).values
        if k < n:
            assert torch.equal(sel_sorted, torch.sort(torch.topk(keys, k).indices).values) or torch.unique(keys).numel() < n
        out2, out3 = torch.empty_like(out), torch.empty_like(out)
        for o, rr in ((out2, r), (out3, torch.rand(4, device=dev, generator=g))):
            _lib.check(lib.fabhip_buffer_sample(_lib.ptr(logw), _lib.ptr(u), _lib.ptr(rr), n, k, _lib.ptr(o), C.c_void_p(wsp), nb,
                                                _lib.stream_ptr()), "buffer_sample")
        assert torch.equal(out, out2) and torch.equal(torch.sort(out3).values, sel_sorted)
        if k >= 300:
            assert not torch.equal(out, out3) and not torch.equal(out, sel_sorted)
            # no trace of the index order: the rank correlation between position and row index is that of a shuffle
            pos = torch.arange(k, device=dev, dtype=torch.float64)
            rk = torch.argsort(torch.argsort(out)).double()
            corr = float(((pos - pos.mean()) * (rk - rk.mean())).sum() / (pos.var(unbiased=False) * k))
            assert abs(corr) < 5.0 / np.sqrt(k)
    # the op (draws from torch's device generator): a set of k distinct valid rows, reproducible under a seed
    torch.manual_seed(5)
    a = ops.buffer_sample_indices(logw, 1)
    logw = torch.randn(70000, device=dev)
    torch.manual_seed(5); a = ops.buffer_sample_indices(logw, 2048)
    torch.manual_seed(5); b = ops.buffer_sample_indices(logw, 2048)
    assert torch.equal(a, b) and a.unique().numel() == 2048 and int(a.min()) >= 0 and int(a.max()) < 70000


@pytest.mark.parametrize("act_norm,clip", [(False, None), (False, 10.0), (True, None)])
def test_one_op_minibatch_step_equals_the_step_by_step_trainer(act_norm, clip):
    """PrioritisedBufferTrainer with every minibatch as ONE `fabhip::buffer_train_step` call against the same trainer stepping
    through the separate ops (tape, torch expressions for the loss weights, parameter gradients, FlatAdam, buffer.adjust): same
    draws, 4 iterations x 3 minibatches - loss, gradient norm, every parameter and the buffer's weights agree to 1e-5."""
    import fab_torch_amd as fa
    from fab_torch_amd.buffer import PrioritisedReplayBuffer
    dev = torch.device("cuda", 0)
    D, K, nodes, M, B = 6, 3, 40, 2, 256
    results = []
    for one_op in (False, True):
        torch.manual_seed(1)
        flow = fa.make_wrapped_normflow_realnvp(D, K, nodes, act_norm=act_norm).to(dev)
        target = fa.ManyWellEnergy(D)
        hmc = fa.HamiltonianMonteCarlo(M, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.1, L=3).to(dev)
        model = fa.FABModel(flow, target, M, alpha=2.0, transition_operator=hmc, loss_type="fab_alpha_div")
        ais = model.annealed_importance_sampler
        opt = fa.FlatAdam(flow, lr=1e-3)

        def init_sampler():
            pt, lw = ais.sample_and_log_weights(B, logging=False)
            return pt.x, lw, pt.log_q
        buf = PrioritisedReplayBuffer(D, 4096, 1024, init_sampler, device=dev)
        tr = fa.PrioritisedBufferTrainer(model, opt, buf, alpha=2.0, n_batches_buffer_sampling=3, max_gradient_norm=5.0,
                                         w_adjust_max_clip=clip)
        tr.one_op_minibatch = one_op
        torch.manual_seed(7)
        infos = [tr.step(i + 1, B) for i in range(4)]
        results.append((infos, torch.cat([p.detach().reshape(-1) for p in flow.parameters()]).clone(), buf.buffer.log_w.clone(),
                        buf.buffer.log_q_old.clone(), tr.last_indices.clone(), int(opt.steps.item())))
    (ia, pa, lwa, lqa, idxa, sa), (ib, pb, lwb, lqb, idxb, sb) = results
    assert torch.equal(idxa, idxb) and sa == sb == 12
    for a, b in zip(ia, ib):
        for key in ("loss", "grad_norm", "w_adjust_mean", "w_adjust_min", "w_adjust_max", "log_q_x_mean", "sampled_log_w_mean",
                    "sampled_log_w_std"):
            assert abs(a[key] - b[key]) <= 1e-5 * max(1.0, abs(a[key])), (key, a[key], b[key])
    assert float((pa - pb).abs().max()) <= 1e-5 * float(pa.abs().max())
    fin = torch.isfinite(lwa)
    assert torch.equal(fin, torch.isfinite(lwb))
    assert float((lwa[fin] - lwb[fin]).abs().max()) <= 1e-4 and float((lqa - lqb).abs().max()) <= 1e-4


def test_one_op_minibatch_step_skips_the_update_on_a_non_finite_loss_and_kills_the_rows():
    """A buffer row whose stored log q is far above the current one gives exp(+large) = inf weight: the loss is not finite, the
    optimiser must not move (reference :172-181) and the step counter must not advance; a row with a non-finite adjustment gets
    log_w = -inf (prioritised_replay_buffer.py:128-131), a finite one - however large - is added."""
    import fab_torch_amd as fa
    from fab_torch_amd import _ops
    dev = torch.device("cuda", 0)
    ops = _ops.load()
    D, K, nodes, B = 6, 3, 40, 64
    flow = _flow(D, K, nodes, dev)
    opt = fa.FlatAdam(flow, lr=1e-2)
    N = 500
    bx = torch.randn(N, D, device=dev)
    blw = torch.zeros(N, device=dev)
    blq = flow.log_prob(bx).detach().clone()
    blq[3] = float("nan")                                   # -> non-finite adjustment: the row is killed
    blq[5] += 500.0                                         # -> w = exp(500) = inf: the loss is not finite
    rows = torch.arange(B, device=dev)
    before = opt.theta.detach().clone()
    packed, _, _, W = flow.native(need_inverse=False)
    with torch.no_grad():
        lq, adj, stats = ops.buffer_train_step(flow._own_handle(), packed, D, K, W, False, bx, rows, blq, True, 2.0, 0.0, blw, blq,
                                               opt.theta.detach(), opt.m, opt.v, 1e-2, 0.9, 0.999, 1e-8, opt.steps, 5.0)
    st = stats.tolist()
    assert not np.isfinite(st[0]) and not np.isfinite(st[5])
    assert torch.equal(opt.theta.detach(), before) and int(opt.steps.item()) == 0
    # (row 5's adjustment, +500, is finite: the reference adds it, :124-127; only the NaN row is killed)
    assert float(blw[3]) == -float("inf") and abs(float(blw[5]) - 500.0) < 1e-2 and float(blw[4]) != -float("inf")
    assert bool(torch.isfinite(blw[6:B]).all()) and torch.equal(blw[B:], torch.zeros(N - B, device=dev))


# ---------------------------------------------------------------------------------------------------------------------------------
# The minibatch arithmetic in the tail of the 8-chain tape kernel (csrc/train_step.hip: k_flow_log_prob_tape_r8, MbTail; the
# reduction mb_finish in csrc/train_kernels.hip) against a plain float64 statement of fab/train_with_prioritised_buffer.py:158-185
# and fab/utils/prioritised_replay_buffer.py:117-131 - on the tail (FABHIP_OPT_TAPE_TILES 0), on the same tiles with
# k_buffer_minibatch as a launch of its own (8) and on the 16-chain tape kernel (16).
# ---------------------------------------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24                                        # unit roundoff of float32
TAIL_SHAPES = {5: [(32, 10, 10), (20, 3, 16), (32, 2, 9)],       # (32, 2, 9): W = 288 padded to 320
               4: [(32, 3, 8), (6, 3, 40), (31, 2, 6)]}          # (31, 2, 6): W = 186 padded to 256, d = 16 and 15 transformed dims
N_BUFFER = 5000


def _tail_cases():
    cases = []
    for G, shapes in TAIL_SHAPES.items():
        for shp in shapes:
            for B in (13, 515):
                cases.append((G, shp, B, 2.0, 10.0))
    for G, shp in ((5, (32, 10, 10)), (4, (6, 3, 40))):
        for B in (2048, 64, 8, 1):
            cases.append((G, shp, B, 2.0, 10.0))
        cases += [(G, shp, 64, 0.5, 10.0), (G, shp, 64, 2.0, "tenth"), (G, shp, 64, 2.0, None), (G, shp, 64, 0.5, "tenth")]
    return cases


def _expected_plan(G, mode):
    return [8 if mode != 16 else 16, G, 1 if mode == 0 else 0]


class _StepCase:
    """One flow + FlatAdam + replay buffer on the device and the float64 oracle of the same flow on the host; `run(mode)` restores
    the start state and makes ONE `fabhip::buffer_train_step` call under FABHIP_OPT_TAPE_TILES = mode."""

    def __init__(self, D, K, nodes, B, seed, lr=1e-3):
        import copy
        import fab_torch_amd as fa
        from helpers import seeded_oracle_flow
        from test_gpu_parity import hip_flow_from_oracle
        self.dev = torch.device("cuda", 0)
        self.D, self.K, self.nodes, self.B, self.lr = D, K, nodes, B, lr
        self.nf = seeded_oracle_flow(D, K, nodes, seed, std=0.05)
        self.nf64 = copy.deepcopy(self.nf).double()
        self.flow = hip_flow_from_oracle(self.nf)
        self.opt = fa.FlatAdam(self.flow, lr=lr)
        self.theta0 = self.opt.theta.detach().clone()
        g = torch.Generator().manual_seed(seed + 7)
        with torch.no_grad():
            self.bx = self.nf.sample_eps(torch.randn(N_BUFFER, D, generator=g))[0] + 0.1 * torch.randn(N_BUFFER, D, generator=g)
        self.rows = torch.randperm(N_BUFFER, generator=g)[:B].contiguous()               # distinct, unsorted
        assert self.rows.unique().numel() == B and (B < 3 or not torch.equal(self.rows, self.rows.sort().values))
        with torch.no_grad():
            self.lq64 = self.nf64.log_prob(self.bx[self.rows].double())
        # stored log q of the minibatch's rows: the current one + N(0, 1) (|adj| stays below 6 |1 - alpha|); the other rows hold
        # values no correct call may read or write
        self.blw = torch.randn(N_BUFFER, generator=g)
        self.blq = 100.0 * torch.randn(N_BUFFER, generator=g)
        self.blq[self.rows] = self.lq64.float() + torch.randn(B, generator=g)

    def run(self, mode, alpha, clip, max_norm=5.0, decisions=True):
        from fab_torch_amd import _ops
        from test_gpu_parity import hip_relu_decisions
        ops, flow, opt, dev = _ops.load(), self.flow, self.opt, self.dev
        with _ops.option(_ops.OPT_TAPE_TILES, mode):
            plan = [int(v) for v in ops.train_step_plan(self.D, self.K, self.D * self.nodes)]
            with torch.no_grad():
                opt.theta.detach().copy_(self.theta0)
                opt.m.zero_(); opt.v.zero_(); opt.steps.zero_()
            flow._packed_key = None
            bx, rows, blw, blq = self.bx.to(dev), self.rows.to(dev), self.blw.to(dev), self.blq.to(dev)
            dec = hip_relu_decisions(flow, bx[rows]) if decisions else None
            packed, D, K, W = flow.native(need_inverse=False)
            with torch.no_grad():
                lq, adj, stats = ops.buffer_train_step(flow._own_handle(), packed, D, K, W, False, bx, rows, blq, True, float(alpha),
                                                       float(clip) if clip is not None else 0.0, blw, blq, opt.theta.detach(), opt.m,
                                                       opt.v, self.lr, 0.9, 0.999, 1e-8, opt.steps, max_norm)
            torch.cuda.synchronize()
            flow._packed_key = None
        return dict(plan=plan, dec=dec, lq=lq.cpu(), adj=adj.cpu(), stats=stats.cpu().double(), blw=blw.cpu(), blq=blq.cpu(),
                    theta=opt.theta.detach().cpu().clone(), m=opt.m.cpu().clone(), v=opt.v.cpu().clone(), steps=int(opt.steps.item()))

    def named_views(self, flat):
        """{oracle parameter name: view of a flat image on the host} (the layout of fabhip_flow_grad_layout)."""
        names = {id(p): n for n, p in self.flow._nf_model.named_parameters()}
        return {names[id(p)]: v for p, v in zip(self.flow._grad_tensors(), self.flow._grad_views(flat))}


_STAT_INDEX = dict(loss=0, w_mean=1, w_min=2, w_max=3, log_q_mean=4)


def _float64_figures(lq, adj, clip):
    """{key: (float64 value, bound)} of the minibatch's logged scalars from the kernel's float32 log q and log_w_adjust, with the
    bounds derived in test_minibatch_tail_against_a_float64_statement_of_the_minibatch; the pre-clip and the clipped weights."""
    B = lq.numel()
    w = torch.exp(adj.double())
    wc = torch.clamp(w, max=clip) if clip is not None else w
    l64 = lq.double()
    e_exp = 4 * 2.0 ** -23
    terms = wc * l64
    # Largest |got - ref| / bound measured on the MI355X over all shapes, clips and tile options (tail and non-tail alike), per B:
    #   B      loss   w_mean  w_min  w_max  log_q_mean        (loss / w_mean: the issue's B x 2^-24 widened by the per-term
    #   1      0.070  0.083   0.093  0.093  0.000              4 x 2^-23 [+ 2^-24]: 10x / 9x the summation bound at B = 1, 2.1x / 2x
    #   8      0.040  0.047   0.037  0.057  0.210              at B = 8, under 15 % from B = 64 on; with the issue's bound alone the
    #   13     0.120  0.086   0.075  0.110  0.088              B = 1 rows would stand at 0.70 / 0.75 of it, every other row lower
    #   64     0.015  0.022   0.113  0.072  0.012              still: the widening is not what makes any case pass)
    #   515    0.004  0.004   0.082  0.112  0.004
    #   2048   0.000  0.001   0.065  0.093  0.001
    return dict(loss=(-terms.sum() / B, (B * U24 + e_exp + U24) * terms.abs().sum() / B),
                w_mean=(w.sum() / B, (B * U24 + e_exp) * w.sum() / B),
                w_min=(w.min(), e_exp * w.min()), w_max=(w.max(), e_exp * w.max()),
                log_q_mean=(l64.sum() / B, B * U24 * l64.abs().sum() / B)), w, wc


def _same_bits(a, b):
    return np.array_equal(a.numpy(), b.numpy(), equal_nan=True)


@pytest.mark.parametrize("G,shape,B,alpha,clip", _tail_cases())
def test_minibatch_tail_against_a_float64_statement_of_the_minibatch(G, shape, B, alpha, clip):
    """ONE `fabhip::buffer_train_step` call from a zeroed optimiser state, on the tail (k_flow_log_prob_tape_r8<G> with MbTail),
    on the same tiles with k_buffer_minibatch as its own launch and on the 16-chain tape, each against the same float64 reference.

    The flow: the returned log q against the float64 oracle at `helpers.close` (1e-4).
    The arithmetic, as a function of the kernel's OWN float32 log q (so that no flow error enters):
      * log_w_adjust and the buffer's new log_w / log_q_old are single float32 operations on known inputs: bit-exact against the
        same torch float32 expressions; every buffer row outside the minibatch comes back untouched.
      * min / max of the pre-clip weight against float64 exp(adj) at 4 x 2^-23 relative (device expf: 1 ulp; the rest is the
        comparison's own rounding).
      * the sums (loss, mean weight, mean log q): float32 summation in any order is within B x 2^-24 of the exact sum, relative to
        the sum of absolute terms.  The terms of mean(log q) are exact inputs: that bound alone.  The terms of the weight sums are
        themselves only known to the expf bound above (4 x 2^-23), those of the loss to that plus one product rounding (2^-24):
        these per-term bounds are added (for B = 1 the summation bound alone is half an ulp, which no 1-ulp expf can meet).
    The gradient: with zero moments and step 0, m after the step is (1 - beta1) x clip_coef x grad and stats[5] the norm; the
    recovered gradient against float64 autograd of -mean(w.detach() log q) through the oracle with the kernel's ReLU decisions
    (w from the kernel's log q) at the criterion of test_flow_parameter_gradients_vs_oracle_autograd; the norm within what that
    criterion implies (|norm a - norm b| <= |a - b|_2 <= sum over tensors sqrt(n) atol + rtol |b|_2); theta after the step
    against float64 Adam on the recovered gradient at 1e-6 absolute."""
    from helpers import close, worst, RTOL
    from test_gpu_parity import fp64_oracle_with_decisions
    D, K, nodes = shape
    case = _StepCase(D, K, nodes, B, seed=400 + D + K + nodes)
    one_minus_alpha = 1.0 - alpha
    tenth = clip == "tenth"
    if tenth:                                   # a clip that catches about a tenth of the rows (from the oracle's log q)
        w_o = torch.exp(one_minus_alpha * (case.lq64 - case.blq[case.rows].double()))
        clip = float(torch.quantile(w_o, 0.9))
    x64 = case.bx[case.rows].double()
    lqo = case.blq[case.rows]
    ref_cache = []                                        # (decisions, log q, gradient by name): one float64 autograd where possible
    for mode in (0, 8, 16):
        r = case.run(mode, alpha, clip)
        assert r["plan"] == _expected_plan(G, mode), (mode, r["plan"])
        lq, st = r["lq"], r["stats"]
        # ---- the flow
        assert close(lq, case.lq64.float(), RTOL), (mode, worst(lq, case.lq64.float()))
        # ---- single float32 operations: bit-exact
        adj = torch.tensor(one_minus_alpha, dtype=torch.float32) * (lq - lqo)
        assert bool(torch.isfinite(adj).all()) and float(adj.abs().max()) < 60.0
        assert torch.equal(r["adj"], adj), mode
        blw, blq = case.blw.clone(), case.blq.clone()
        blw[case.rows] = case.blw[case.rows] + adj
        blq[case.rows] = lq
        assert torch.equal(r["blw"], blw) and torch.equal(r["blq"], blq), mode
        # ---- statistics in float64 from the kernel's log q
        figures, w, wc = _float64_figures(lq, adj, clip)
        for key, (ref, tol) in figures.items():
            got = st[_STAT_INDEX[key]]
            print(f"TAIL {shape} B={B} alpha={alpha} clip={clip} tiles={mode} {key}: |got - ref| = {abs(float(got - ref)):.3e} "
                  f"= {abs(float(got - ref)) / float(tol):.3f} x bound")
            assert abs(float(got - ref)) <= float(tol), (mode, key, float(got), float(ref), float(tol))
        if tenth:
            assert 0 < int((w > clip).sum()) <= B // 4     # the clip acts, on about a tenth of the rows
        # ---- the gradient, recovered from Adam's first moment
        assert r["steps"] == 1
        norm32 = np.float32(float(st[5]))
        coef32 = min(np.float32(1.0), np.float32(5.0) / (norm32 + np.float32(1e-6)))
        one_m_b1 = np.float32(1.0) - np.float32(0.9)
        g_rec = r["m"].double() / (float(one_m_b1) * float(coef32))
        ref = next((c for c in ref_cache if torch.equal(c[1], lq) and all(
            torch.equal(a1, b1) and torch.equal(a2, b2) for (a1, a2), (b1, b2) in zip(c[0], r["dec"]))), None)
        if ref is None:
            nf64 = fp64_oracle_with_decisions(case.nf, r["dec"])
            loss = -(wc.detach() * nf64.log_prob(x64)).mean()
            names = [n for n, _ in nf64.named_parameters()]
            grads = torch.autograd.grad(loss, [p for _, p in nf64.named_parameters()])
            ref = (r["dec"], lq, dict(zip(names, grads)))
            ref_cache.append(ref)
        views = case.named_views(g_rec)
        assert set(views) == set(ref[2])
        norm_sq, slack = 0.0, 0.0
        for name, b in ref[2].items():
            a = views[name].reshape(b.shape)
            assert close(a.float(), b.float(), RTOL, atol_scale=30), f"tiles={mode} {name}: {worst(a.float(), b.float()):.2f} x tolerance"
            norm_sq += float((b * b).sum())
            slack += float(np.sqrt(b.numel())) * 30 * 2e-6 * max(1.0, float(b.abs().max()))
        assert abs(float(st[5]) - np.sqrt(norm_sq)) <= slack + RTOL * np.sqrt(norm_sq), (mode, float(st[5]), np.sqrt(norm_sq))
        # ---- theta after the step: float64 Adam (the kernel's float32 hyper-parameters) on the recovered gradient
        b1, b2, lr, eps = float(np.float32(0.9)), float(np.float32(0.999)), float(np.float32(case.lr)), float(np.float32(1e-8))
        gc = g_rec * float(coef32)
        m64, v64 = (1 - b1) * gc, (1 - b2) * gc * gc
        theta = case.theta0.cpu().double() - (lr / (1 - b1)) * m64 / (v64.sqrt() / np.sqrt(1 - b2) + eps)
        assert float((r["theta"].double() - theta).abs().max()) <= 1e-6, (mode, float((r["theta"].double() - theta).abs().max()))
    assert len(ref_cache) <= 2                            # (tiles 0 and 8 are the same forward: one reference serves both)


NONFINITE_CASES = ["nan_log_q_old_first", "nan_log_q_old_middle", "nan_log_q_old_last", "pos_and_neg_inf_log_q_old", "overflowing_weight",
                   "x_far_out", "overflowing_weight_without_clip"]


@pytest.mark.parametrize("kind", NONFINITE_CASES)
@pytest.mark.parametrize("G,shape", [(4, (6, 3, 40)), (5, (20, 3, 16))])
def test_minibatch_step_with_non_finite_rows_follows_the_reference(G, shape, kind):
    """Non-finite inputs on the tail and on the two non-tail paths, against oracle/train.py's Buffer.adjust and
    train_with_prioritised_buffer.py:164-181 evaluated with torch on the kernel's own log q: which rows are killed and which
    adjusted (bit-exact), loss / min / max NaN-or-inf exactly as torch.mean / torch.min / torch.max give them (a NaN weight in the
    first, a middle and the last 8-row workgroup makes min and max NaN), parameters and step counter unmoved when the reference
    skips the update and moved when it steps.  The non-finite rows are non-finite by construction (NaN, inf, |adj| = 500); every
    other row has |adj| < 60, so no case depends on where float32 exp overflows."""
    from helpers import close, RTOL
    from oracle.train import Buffer
    D, K, nodes = shape
    B, alpha = 64, 2.0
    case = _StepCase(D, K, nodes, B, seed=500 + D + K + nodes)
    clip, special = 10.0, []
    r_ = case.rows
    if kind.startswith("nan_log_q_old"):
        special = [{"first": 0, "middle": 29, "last": B - 1}[kind.rsplit("_", 1)[1]]]
        case.blq[r_[special[0]]] = float("nan")
    elif kind == "pos_and_neg_inf_log_q_old":
        special = [5, 40]
        case.blq[r_[5]], case.blq[r_[40]] = float("inf"), -float("inf")
    elif kind.startswith("overflowing_weight"):
        special = [5]
        case.blq[r_[5]] += 500.0
        clip = None if kind.endswith("without_clip") else 10.0
    elif kind == "x_far_out":
        special = [17]
        case.bx[r_[17]] = 1e30
        with torch.no_grad():
            case.lq64 = case.nf64.log_prob(case.bx[r_].double())
        assert not bool(torch.isfinite(case.lq64[17]))     # not finite in the float64 oracle either
    others = torch.ones(B, dtype=torch.bool)
    others[special] = False
    for mode in (0, 8, 16):
        r = case.run(mode, alpha, clip, decisions=False)
        assert r["plan"] == _expected_plan(G, mode), (mode, r["plan"])
        lq, st = r["lq"], r["stats"]
        assert close(lq[others], case.lq64.float()[others], RTOL), mode
        lqo = case.blq[r_]
        adj = torch.tensor(1.0 - alpha, dtype=torch.float32) * (lq - lqo)
        assert float(adj[others].abs().max()) < 60.0
        assert all((not np.isfinite(float(adj[i]))) or abs(float(adj[i])) > 200.0 for i in special)
        assert _same_bits(r["adj"], adj), mode
        ob = Buffer(D, N_BUFFER, 1)
        ob.log_w, ob.log_q_old = case.blw.clone(), case.blq.clone()
        ob.adjust(adj, lq, r_)
        assert _same_bits(r["blw"], ob.log_w) and _same_bits(r["blq"], ob.log_q_old), mode
        killed = [i for i in range(B) if float(r["blw"][r_[i]]) == -float("inf")]
        assert killed == [i for i in special if not (np.isfinite(float(adj[i])) and np.isfinite(float(lq[i])))], (mode, killed)
        # the reference's scalars with torch on the host
        w_pre = torch.exp(adj)
        w = torch.clip(w_pre, max=clip) if clip is not None else w_pre
        loss = -torch.mean(w * lq)
        figures = _float64_figures(lq, adj, clip)[0]
        for key, ref in (("loss", loss), ("w_mean", w_pre.mean()), ("w_min", w_pre.min()), ("w_max", w_pre.max()),
                         ("log_q_mean", lq.mean())):
            got, ref = float(st[_STAT_INDEX[key]]), float(ref)
            if np.isfinite(ref):                           # (then every term is finite: the float64 value and its derived bound)
                ref64, tol = figures[key]
                assert np.isfinite(got) and abs(got - float(ref64)) <= float(tol), (mode, kind, key, got, float(ref64), float(tol))
            else:                                          # NaN where torch gives NaN, the same infinity where it gives one
                assert (np.isnan(got) and np.isnan(ref)) or got == ref, (mode, kind, key, got, ref)
        skipped = bool(torch.isnan(loss) or torch.isinf(loss))
        assert skipped == (kind not in ("pos_and_neg_inf_log_q_old", "overflowing_weight"))
        if skipped:
            assert torch.equal(r["theta"], case.theta0.cpu()) and r["steps"] == 0 and not bool(r["m"].any()) and not bool(r["v"].any())
            assert np.isnan(float(st[5]))                  # the op's "no norm was computed" (the trainer then keeps its last one)
        else:
            assert r["steps"] == 1 and np.isfinite(float(st[5])) and bool(torch.isfinite(r["theta"]).all())
            assert not torch.equal(r["theta"], case.theta0.cpu()) and bool(r["m"].any())


def test_train_step_plan_reports_the_tail_only_where_the_dispatcher_fuses_it():
    """fabhip::train_step_plan = the dispatcher's own decision: tail at every 8-chain shape with FABHIP_OPT_TAPE_TILES = 0, never
    with 8 or 16, never at a shape without the 8-chain image (the recorded trainer traces g12: D = 6, W = 30; D > 32; W = 512)."""
    from fab_torch_amd import _ops
    ops = _ops.load()
    for mode in (0, 8, 16):
        with _ops.option(_ops.OPT_TAPE_TILES, mode):
            for G, shapes in TAIL_SHAPES.items():
                for D, K, nodes in shapes:
                    assert [int(v) for v in ops.train_step_plan(D, K, D * nodes)] == _expected_plan(G, mode)
            for D, K, W in ((6, 3, 30), (60, 3, 240), (32, 2, 512), (32, 10, 128)):
                plan = [int(v) for v in ops.train_step_plan(D, K, W)]
                assert plan[0] == 16 and plan[2] == 0, (D, K, W, plan)


def _skip_scenario(path):
    """A trainer on `path` through (a) a first iteration whose minibatches are all skipped, and - from a fresh state - (b) an iteration
    whose LAST minibatch is skipped, (c) an iteration whose minibatches are all skipped; the assertions that do not compare paths."""
    import fab_torch_amd as fa
    from fab_torch_amd import _ops
    from fab_torch_amd.buffer import PrioritisedReplayBuffer
    dev = torch.device("cuda", 0)
    D, K, nodes, M, B, nb = 6, 3, 40, 2, 256, 3
    assert [int(v) for v in _ops.load().train_step_plan(D, K, D * nodes)][2] == 1
    nan = float("nan")

    def make():
        torch.manual_seed(1)
        flow = fa.make_wrapped_normflow_realnvp(D, K, nodes, act_norm=False).to(dev)
        target = fa.ManyWellEnergy(D)
        hmc = fa.HamiltonianMonteCarlo(M, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.1, L=3).to(dev)
        model = fa.FABModel(flow, target, M, alpha=2.0, transition_operator=hmc, loss_type="fab_alpha_div")
        ais = model.annealed_importance_sampler
        opt = torch.optim.Adam(flow.parameters(), lr=1e-3) if path == "torch_adam" else fa.FlatAdam(flow, lr=1e-3)

        def init_sampler():
            pt, lw = ais.sample_and_log_weights(B, logging=False)
            return pt.x, lw, pt.log_q
        buf = PrioritisedReplayBuffer(D, 4096, 1024, init_sampler, device=dev)
        tr = fa.PrioritisedBufferTrainer(model, opt, buf, alpha=2.0, n_batches_buffer_sampling=nb, max_gradient_norm=5.0,
                                         w_adjust_max_clip=10.0)
        tr.one_op_minibatch = path == "one_op"
        return flow, opt, buf, tr

    def params(flow):
        return torch.cat([p.detach().reshape(-1) for p in flow.parameters()]).clone()

    def steps(opt):
        if path != "torch_adam":
            return int(opt.steps.item())
        return int(max(float(s["step"]) for s in opt.state.values())) if opt.state else 0

    def poison_minibatches(buf, which, originals=None):
        """Every row of the minibatches `which` gets a NaN stored log q as it is sampled (in the buffer for the one-op path, which
        reads it there; in the gathered copies for the other two)."""
        o_idx, o_nb = originals or (buf.sample_indices, buf.sample_n_batches)

        def sample_indices(n, **kw):
            idx = o_idx(n, **kw)
            for j in which:
                buf.buffer.log_q_old[torch.chunk(idx, nb)[j]] = nan
            return idx

        def sample_n_batches(**kw):
            out = [list(m) for m in o_nb(**kw)]
            for j in which:
                out[j][2] = torch.full_like(out[j][2], nan)
            return [tuple(m) for m in out]
        buf.sample_indices, buf.sample_n_batches = sample_indices, sample_n_batches
        return o_idx, o_nb

    # (a) no norm exists yet: every minibatch of the first iteration is skipped -> NaN, nothing moves
    flow, opt, buf, tr = make()
    before = params(flow)
    poison_minibatches(buf, range(nb))
    torch.manual_seed(7)
    info = tr.step(1, B)
    assert np.isnan(info["loss"]) and np.isnan(info["grad_norm"])
    assert torch.equal(params(flow), before) and steps(opt) == 0
    # (b) the LAST minibatch is skipped: the norm of the one before it is logged
    flow, opt, buf, tr = make()
    originals = poison_minibatches(buf, [nb - 1])
    torch.manual_seed(7)
    info_b = tr.step(1, B)
    assert np.isnan(info_b["loss"]) and np.isfinite(info_b["grad_norm"]) and info_b["grad_norm"] > 0
    assert steps(opt) == nb - 1
    if path == "one_op":
        per = tr.minibatch_stats()
        assert [s["norm_computed"] for s in per] == [True] * (nb - 1) + [False]
        assert info_b["grad_norm"] == per[nb - 2]["grad_norm"] == per[nb - 1]["grad_norm"]
    after_b = params(flow)
    # (c) then a whole iteration is skipped: the norm of iteration (b) is still the logged one, nothing moves
    poison_minibatches(buf, range(nb), originals)
    info_c = tr.step(2, B)
    assert np.isnan(info_c["loss"]) and info_c["grad_norm"] == info_b["grad_norm"]
    assert torch.equal(params(flow), after_b) and steps(opt) == nb - 1
    return info_b["grad_norm"]


@pytest.mark.parametrize("path", ["one_op", "flat_adam_step_by_step", "torch_adam"])
def test_logged_gradient_norm_on_a_skipped_minibatch_is_the_last_computed_one(path):
    """train_with_prioritised_buffer.py:172-198: a minibatch with a non-finite loss computes no gradient norm, so the iteration logs
    the last one that WAS computed - within the iteration, or in an earlier iteration (the reference's variable lives across its
    loop); NaN only where none exists yet.  On all three paths (the one-op step with the tail, FlatAdam through the separate ops,
    torch Adam through autograd); the update of the skipped minibatch is skipped as before, and the paths log the same norm
    (same seeds, same draws: 1e-4 relative, the criterion of the teacher-forced trainer replays)."""
    norm = _skip_scenario(path)
    if path != "one_op":
        ref = _skip_scenario("one_op")
        assert abs(norm - ref) <= 1e-4 * ref, (path, norm, ref)
