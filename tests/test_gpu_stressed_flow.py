"""The RealNVP kernels on flows that have left their initialisation (tests/stressed_flow.py): every InvertibleAffine a
non-orthogonal LU factorisation with a real permutation and pivots of both signs, hidden Linears, last Linears, base and ActNorm
re-drawn.  Yardstick: the float64 copy of the oracle flow; the fp32 oracle on the same inputs is the measure of what float32 can do.

ROW RULE.  Errors are |a - f64| / scale, scale = max(1, max|f64|) of the case.  A row passes by
  (i)   `helpers.close` at RTOL (1e-4 |b| + 2e-6 scale per element),
  (ii)  HIP's error on the row <= 4x the fp32 oracle's error on that row,
  (iii) (gradients, and what an HMC step makes of them) HIP's error <= 4x `spread`: the largest move of the float64 result over 8
        copies of the row whose input is perturbed by 2.4e-7 relative - the conditioning probe and the 4x of
        test_gpu_parity.test_headline_architecture_vs_reference_golden.  Rows that pass by (iii) only are counted: at most B // 8
        per case, together with the accept decisions that differ inside the rounding band of their threshold.
Values (log q, x, z) use (i) and (ii) only.  test_stressed_flow.py holds the fp32 oracle alone to the same rule on every case.

Groups: (a) the affine maps alone (last Linears zero), (b) density / gradient / sample on the 16-chain kernels, (c) the 8- and
4-chain families incl. one teacher-forced HMC transition, (d) parameter gradients of the density direction on every tape path,
(e) the sampling backward.  In (d) and (e) the float64 oracle applies the ReLU decisions HIP took (read from its tape), so no row
is excused; a tensor passes by the tolerance of test_flow_parameter_gradients_vs_oracle_autograd or by clause (ii) against the fp32
oracle under the same decisions.

Levels left out because the fp32 ORACLE leaves the rule there (test_stressed_flow.py, stressed_flow.AFFINE_DENSITY_MAX_COND):
group (a) checks log q and d log q / dx at 1e2 per layer only - x -> z multiplies the input's rounding by cond^K and at 1e4 the fp32
oracle's log q is hundreds to thousands of tolerance units from float64; the sampling direction is checked at 1e2 and 1e4.

Measured on one MI355X (worst row of the group, tolerance units of clause (i): HIP / fp32 oracle; rows by (iii) only, worst case):
see tests/README.md."""
import copy
import functools

import numpy as np
import pytest
import torch

import stressed_flow as sf
from helpers import close, worst, RTOL
from test_gpu_parity import FLOW_CASES, hip_relu_decisions, _ForcedReLU, DEV

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops            # noqa: E402
from oracle import ais as oais            # noqa: E402
from oracle import flow as oflow          # noqa: E402
from oracle import targets as otgt        # noqa: E402

B, RAGGED = sf.B, 37
CAP = lambda n: n // 8                    # noqa: E731


def test_the_shapes_are_the_ones_of_the_suite():
    assert [c[:3] for c in FLOW_CASES] == sf.FLOW_SHAPES


def hip_flow(nf):
    """test_gpu_parity.hip_flow_from_oracle for flows with or without ActNorm: `load_state_dict` of the stressed oracle (P and
    sign_S travel as buffers)."""
    an = any(isinstance(f, oflow.ActNorm) for f in nf.flows)
    D = nf.q0.loc.shape[1]
    K = sum(isinstance(f, oflow.InvertibleAffine) for f in nf.flows)
    W = nf.flows[0].flows[1].param_map.net[0].weight.shape[0]
    f = fa.RealNVP(D, K, W // D, act_norm=an)
    res = f._nf_model.load_state_dict(nf.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return f.to(DEV).requires_grad_(False)


@functools.lru_cache(maxsize=4)
def case(D, K, nodes, cond, s_max, act_norm=False, n=B):
    """The oracle side of one case, computed once and shared by the tests (and tile shapes) that use it; never modified."""
    return sf.oracle_case(D, K, nodes, cond, s_max, act_norm, n)


def lazy_grad_spread(c):
    """clause (iii)'s probe for the rows that ask for it."""
    scale = max(1.0, float(c["g64"].abs().max()))

    def f(rows):
        return sf.grad_spread(c["nf64"], c["x"][rows], c["g64"][rows], scale, seed=int(rows[0]))
    return f


def check_density_and_sample(c, hf, n, density=True, sample=True, full=True):
    """native_sample, log_prob_and_grad, log_prob and the differentiable log_prob of `hf` against the float64 oracle of case `c`."""
    report = []
    if sample:
        x_h, ls_h = hf.native_sample(c["eps"].to(DEV))
        report.append(sf.row_rule("sample x", x_h, c["xs32"], c["xs64"]))
        report.append(sf.row_rule("sample log q", ls_h, c["ls32"], c["ls64"]))
    if density:
        xd = c["x"].float().to(DEV)
        lq_h, g_h = hf.log_prob_and_grad(xd)
        report.append(sf.row_rule("log q", lq_h, c["lq32"], c["lq64"]))
        report.append(sf.row_rule("d log q / dx", g_h, c["g32"], c["g64"], spread=lazy_grad_spread(c), cap=CAP(n)))
        if full:
            report.append(sf.row_rule("log_prob", hf.log_prob(xd), c["lq32"], c["lq64"]))
            hf.requires_grad_(True)
            try:
                xg = xd.clone().requires_grad_(True)
                lq_t = hf.log_prob(xg)
                assert lq_t.requires_grad
                (g_t,) = torch.autograd.grad(lq_t.sum(), xg)
            finally:
                hf.requires_grad_(False)
            report.append(sf.row_rule("differentiable log q", lq_t.detach(), c["lq32"], c["lq64"]))
            report.append(sf.row_rule("its d log q / dx", g_t, c["g32"], c["g64"], spread=lazy_grad_spread(c), cap=CAP(n)))
    for r in report:
        print(r[1])
    return report


# ---- (a) the affine maps alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cond", sf.AFFINE_CONDS)
@pytest.mark.parametrize("D,K,nodes", sf.AFFINE_SHAPES)
def test_affine_maps_alone(D, K, nodes, cond):
    """Last Linears zero: sample and density are the product of the K affine maps, so a wrong triangle, sign or permutation is an
    O(1) error here and nothing downstream can hide it.  k_affine_assemble builds W^-1 as the reference does (float64 triangular
    inverses cast to fp32, fp32 products): clause (ii) is the fair bound."""
    c = case(D, K, nodes, cond ** K, 0.0)
    hf = hip_flow(c["nf"])
    check_density_and_sample(c, hf, B, density=cond <= sf.AFFINE_DENSITY_MAX_COND)


def test_affine_maps_alone_ragged_batch():
    c = case(32, 2, 1, 1e2 ** 2, 0.0, False, RAGGED)
    check_density_and_sample(c, hip_flow(c["nf"]), RAGGED)


# ---- (b) density, gradient and sample on the 16-chain kernels ------------------------------------------------------------------------
def _b_cases():
    out = []
    for shp in sf.FLOW_SHAPES:
        out += [shp + lv + (False,) for lv in sf.LEVELS if shp + lv not in sf.DROPPED]
        out.append(shp + (100.0, 1.0, True))
    return out


@pytest.mark.parametrize("D,K,nodes,cond,s_max,act_norm", _b_cases())
def test_density_gradient_sample(D, K, nodes, cond, s_max, act_norm):
    c = case(D, K, nodes, cond, s_max, act_norm)
    check_density_and_sample(c, hip_flow(c["nf"]), B)


@pytest.mark.parametrize("act_norm", [False, True])
def test_density_gradient_sample_ragged_batch(act_norm):
    c = case(32, 10, 10, 100.0, 1.0, act_norm, RAGGED)
    check_density_and_sample(c, hip_flow(c["nf"]), RAGGED)


# ---- (c) the 8- and 4-chain families -----------------------------------------------------------------------------------------------
HMC_EPS, HMC_L, HMC_BETA = 0.2, 3, 0.25      # (beta = 0.25, alpha = 2: log q and log p enter the annealed density with 0.5 each)


@functools.lru_cache(maxsize=2)
def hmc_case(D, K, nodes, cond, s_max, n=B):
    """One HMC transition on ManyWell(D) in float64 and by the fp32 oracle, both from the float64 oracle's point at the density
    points of the case, same momentum and exponential noise."""
    c = case(D, K, nodes, cond, s_max, False, n)
    tgt = otgt.ManyWell(D)
    g = torch.Generator().manual_seed(77 + D + K)
    noise_p = torch.randn(1, n, D, generator=g)
    noise_e = torch.empty(1, n).exponential_(generator=g)
    p64 = oais.create_point(c["x"], c["nf64"].log_prob, tgt.log_prob, True)
    # the step sizes as float32 holds them (the device keeps them in float32)
    proto = oais.HMC(1, D, None, None, alpha=2.0, epsilon=HMC_EPS, L=HMC_L)

    def run(nf, dtype, pt, npz, nez):
        h = oais.HMC(1, D, nf.log_prob, tgt.log_prob, alpha=2.0, p_target=False, epsilon=HMC_EPS, L=HMC_L, eval_mode=True, dtype=dtype)
        h.epsilons, h.common_epsilon = proto.epsilons.to(dtype).clone(), proto.common_epsilon.to(dtype).clone()
        out = h.transition(pt, 1, HMC_BETA, npz.to(dtype), nez.to(dtype))
        return out, h
    o64, h64 = run(c["nf64"], torch.float64, p64.clone(), noise_p, noise_e)
    p32 = oais.Point(*(t.float() for t in (p64.x, p64.log_q, p64.log_p, p64.grad_log_q, p64.grad_log_p)))
    o32, _ = run(c["nf"], torch.float32, p32, noise_p, noise_e)

    def spread(rows):
        """per row: the largest move of (x, log q, log p) after the float64 transition over 8 copies whose state and momentum noise
        are perturbed by 2.4e-7 relative (the probe of test_headline_architecture_vs_reference_golden), each in its own scale."""
        rows = np.asarray(rows)
        gen = torch.Generator().manual_seed(1000 + int(rows[0]))
        x0 = c["x"][rows].repeat_interleave(8, 0)
        n0 = noise_p[0, rows].double().repeat_interleave(8, 0)
        x0 = x0 * (1 + sf.PROBE * torch.randn(x0.shape, generator=gen, dtype=torch.float64))
        n0 = n0 * (1 + sf.PROBE * torch.randn(n0.shape, generator=gen, dtype=torch.float64))
        pp = oais.create_point(x0, c["nf64"].log_prob, tgt.log_prob, True)
        e8 = noise_e[0, rows].double().repeat_interleave(8, 0)[None]
        out, _ = run(c["nf64"], torch.float64, pp, n0[None], e8)
        res = {}
        for k, a, b in (("x", out.x, o64.x), ("log_q", out.log_q, o64.log_q), ("log_p", out.log_p, o64.log_p)):
            sc = max(1.0, float(b.abs().max()))
            d = (a.view(len(rows), 8, -1) - b[rows].view(len(rows), 1, -1)).abs().amax(dim=(1, 2)) / sc
            res[k] = d.numpy()
        return res
    return dict(p64=p64, o64=o64, o32=o32, margin=h64.last_margin.clone(), accept=h64.last_accept.clone(), noise_p=noise_p,
                noise_e=noise_e, eps=proto.epsilons.clone(), ceps=proto.common_epsilon.clone(), spread=spread)


def _c_cases():
    return [shp + lv for shp in sf.SMALL_TILE_SHAPES for lv in sf.small_tile_levels(shp)]


@pytest.mark.parametrize("shape", [4, 8, 16])
@pytest.mark.parametrize("D,K,nodes,cond,s_max", _c_cases())
def test_small_tile_families(D, K, nodes, cond, s_max, shape):
    """`fa.create_point` (log q, grad log q), the flow sample and one HMC transition under FABHIP_OPT_TILE_SHAPE 4 / 8 / 16: the
    fused-stage kernels form A_k[:, :d] W1^T at pack time - here for the first time with a non-orthogonal A_k.  Includes D = 32,
    K = 10, W = 320 at all three levels and W = 512 (where the small tiles have no image and the call must still be right)."""
    check_small_tiles(D, K, nodes, cond, s_max, shape, B)


@pytest.mark.parametrize("shape", [4, 8, 16])
def test_small_tile_families_ragged_batch(shape):
    check_small_tiles(32, 10, 10, 100.0, 1.0, shape, RAGGED)


def check_small_tiles(D, K, nodes, cond, s_max, shape, n):
    c = case(D, K, nodes, cond, s_max, False, n)
    hc = hmc_case(D, K, nodes, cond, s_max, n)
    hf = hip_flow(c["nf"])
    target = fa.ManyWellEnergy(D)
    with _ops.option(_ops.OPT_TILE_SHAPE, shape):
        pt = fa.create_point(c["x"].float().to(DEV), hf, target, with_grad=True)
        x_h, ls_h = hf.native_sample(c["eps"].to(DEV))
        hmc = fa.HamiltonianMonteCarlo(1, D, hf.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=HMC_EPS, L=HMC_L,
                                       eval_mode=True).to(DEV)
        hmc.epsilons.copy_(hc["eps"]); hmc.common_epsilon.copy_(hc["ceps"])
        p64 = hc["p64"]
        start = fa.Point(*(t.float().to(DEV) for t in (p64.x, p64.log_q, p64.log_p, p64.grad_log_q, p64.grad_log_p)))
        x_in = start.x.clone()
        out = hmc.transition(start, 1, HMC_BETA, noise_p=hc["noise_p"].to(DEV), noise_e=hc["noise_e"].to(DEV))
        torch.cuda.synchronize()
    rep = [sf.row_rule("create_point log q", pt.log_q, c["lq32"], c["lq64"]),
           sf.row_rule("create_point grad log q", pt.grad_log_q, c["g32"], c["g64"], spread=lazy_grad_spread(c), cap=CAP(n)),
           sf.row_rule("sample x", x_h, c["xs32"], c["xs64"]),
           sf.row_rule("sample log q", ls_h, c["ls32"], c["ls64"])]
    for r in rep:
        print(r[1])
    # the transition
    o64, o32 = hc["o64"], hc["o32"]
    acc_h = (out.x != x_in).any(1).cpu()
    differ = (acc_h != hc["accept"]).numpy()
    hs = (o64.log_q.abs() + o64.log_p.abs()).clamp(min=1.0)
    band = (64 * 1.1920929e-07 * 3 * hs).numpy()
    m = hc["margin"].numpy()
    # (a non-finite float64 margin is a rejected proposal: it lies in no band, so HIP has to reject it as well)
    outside = differ & ~(np.abs(m) <= band)
    assert not outside.any(), (f"{int(outside.sum())} accept decisions differ from float64 outside the rounding band: rows "
                               f"{np.nonzero(outside)[0][:8].tolist()}, margins {m[outside][:8]}, bands {band[outside][:8]}")
    same = torch.tensor(~differ)
    only3 = np.zeros(int(same.sum()), dtype=bool)
    idx = np.nonzero(~differ)[0]
    for k, a, b32, b64 in (("x", out.x, o32.x, o64.x), ("log_q", out.log_q, o32.log_q, o64.log_q), ("log_p", out.log_p, o32.log_p, o64.log_p)):
        # (scale of the whole case: the rule's, also for the rows compared)
        sp = lambda rows, k=k: hc["spread"](idx[rows])[k]                       # noqa: E731
        r = sf.row_rule(f"HMC {k}", a.cpu()[same], b32[same], b64[same], spread=sp, scale_of=b64)
        print(r[1])
        only3 |= r[0]
    n_soft = int(only3.sum()) + int(differ.sum())
    print(f"HMC: {int(hc['accept'].sum())} of {n} accepted in float64, {int(differ.sum())} decisions differ inside the band, "
          f"{int(only3.sum())} rows by (iii) only")
    assert n_soft <= CAP(n), f"{int(only3.sum())} rows by clause (iii) only + {int(differ.sum())} flipped decisions > {CAP(n)}"


# ---- (d) parameter gradients of the density direction ----------------------------------------------------------------------------------
def forced(nf, decisions, dtype):
    """The oracle flow (with or without ActNorm) whose ReLUs apply the given decisions, in float64 or float32."""
    m = copy.deepcopy(nf).to(dtype)
    blocks = [f for f in m.flows if isinstance(f, oflow.AffineCouplingBlock)]
    for blk, (m1, m2) in zip(blocks, decisions):
        net = blk.flows[1].param_map.net
        net[1], net[3] = _ForcedReLU(m1), _ForcedReLU(m2)
    return m


def judge_tensors(names, g_h, g_32, g_64):
    """Per parameter tensor: the tolerance of test_flow_parameter_gradients_vs_oracle_autograd (close at RTOL, floor x 30), or
    clause (ii): HIP's largest error on the tensor <= 4x the fp32 oracle's under the same decisions.  L, U, log_S on their own."""
    lines, bad = [], []
    for n, a, b32, b64 in zip(names, g_h, g_32, g_64):
        a, b32, b64 = a.detach().cpu().double(), b32.detach().double(), b64.detach()
        assert a.shape == b64.shape, n
        assert bool(torch.isfinite(a).all()), f"{n}: non-finite gradient"
        sc = max(1.0, float(b64.abs().max()))
        eh, eo = float((a - b64).abs().max()) / sc, float((b32 - b64).abs().max()) / sc
        ok = close(a, b64, RTOL, atol_scale=30) or eh <= 4 * eo
        lines.append(f"{n}: HIP {worst(a, b64):.2f} fp32 oracle {worst(b32, b64):.2f} tol units")
        if not ok:
            bad.append(lines[-1] + f" (errors {eh:.2e} / {eo:.2e} of the scale)")
    lu = [l for l in lines if l.split(":")[0].rsplit(".", 1)[-1] in ("L", "U", "log_S")]
    print("; ".join(lu))
    assert not bad, "\n".join(bad)
    assert any(n.endswith(".L") for n in names) and any(n.endswith(".log_S") for n in names)
    return lines


def _grads(flow, params, x, coef):
    for p in params:
        p.grad = None
    xg = x.clone().requires_grad_(True)
    lq = flow.log_prob(xg)
    (lq * coef).sum().backward()
    return lq.detach(), [p.grad.detach().clone() for p in params], xg.grad.detach()


EIGHT_CHAIN_TAPE = {(32, 10, 10), (6, 8, 40)}          # shapes with the 8-chain stream tape (test_gpu_train_step.TAIL_SHAPES' widths)


def _d_cases():
    out = []
    for shp in sf.PARAM_GRAD_SHAPES:
        for lv in sf.LEVELS[1:]:
            if shp + lv in sf.DROPPED:
                continue
            for mode, pgrad in ((0, 1), (8, 1), (16, 1), (16, 0)) if shp in EIGHT_CHAIN_TAPE else ((0, 1), (0, 0)):
                out.append(shp + lv + (mode, pgrad))
    return out


@pytest.mark.parametrize("D,K,nodes,cond,s_max,mode,pgrad", _d_cases())
def test_parameter_gradients_of_the_density(D, K, nodes, cond, s_max, mode, pgrad):
    """sum_b coef_b d log q(x_b) / d theta on every tape path: 8-chain stream tape (FABHIP_OPT_TAPE_TILES 0 / 8) and 16-chain tape
    (16, and the default wherever no 8-chain image exists) with the tile GEMM, the 16-chain tape with the block kernel
    (FABHIP_OPT_PGRAD 0).  The first check of k_affine_grads (chain rule to L, U, log_S) off the orthogonal point."""
    check_param_grads(D, K, nodes, cond, s_max, mode, pgrad, B)


@pytest.mark.parametrize("mode", [0, 16])
def test_parameter_gradients_of_the_density_ragged_batch(mode):
    check_param_grads(32, 10, 10, 100.0, 1.0, mode, 1, RAGGED)


def check_param_grads(D, K, nodes, cond, s_max, mode, pgrad, n):
    c = case(D, K, nodes, cond, s_max, False, n)
    nf = c["nf"]
    hf = hip_flow(nf).requires_grad_(True)
    xd = c["x"].float().to(DEV)
    coef = torch.randn(n, generator=torch.Generator().manual_seed(11)) / n
    with _ops.option(_ops.OPT_TAPE_TILES, mode), _ops.option(_ops.OPT_PGRAD, pgrad):
        plan = [int(v) for v in _ops.load().train_step_plan(D, K, D * nodes)]
        want = 8 if ((D, K, nodes) in EIGHT_CHAIN_TAPE and mode != 16) else 16
        assert plan[0] == want, f"tape tiles {plan[0]}, expected {want} (plan {plan})"
        dec = hip_relu_decisions(hf, xd)
        names = [k for k, _ in nf.named_parameters()]
        hp = dict(hf._nf_model.named_parameters())
        assert set(hp) == set(names)
        lq_h, g_h, gx_h = _grads(hf, [hp[k] for k in names], xd, coef.to(DEV))
        torch.cuda.synchronize()
    nf64, nf32 = forced(nf, dec, torch.float64), forced(nf, dec, torch.float32)
    lq_64, g_64, gx_64 = _grads(nf64, [p for _, p in nf64.named_parameters()], c["x"], coef.double())
    lq_32, g_32, gx_32 = _grads(nf32, [p for _, p in nf32.named_parameters()], c["x"].float(), coef)
    print(sf.row_rule("log q", lq_h, lq_32, lq_64)[1])
    print(sf.row_rule("d loss / dx", gx_h, gx_32, gx_64)[1])            # no clause (iii): the decisions are HIP's own
    judge_tensors(names, g_h, g_32, g_64)


# ---- (e) the sampling backward ---------------------------------------------------------------------------------------------------------
def sample_tape_decisions(hf, x_dev):
    """The ReLU decisions of the sampling backward: fabhip_flow_sample_grad_tape writes the tape of the density direction (same
    layout), H1 / H2 after the ReLU."""
    ops = _ops.load()
    packed, D, K, W = hf.native()
    n = x_dev.shape[0]
    tape, _ = ops.realnvp_sample_grad_tape(packed, D, K, W, x_dev, torch.zeros_like(x_dev), torch.ones(n, device=x_dev.device))
    lay = [int(v) for v in ops.flow_tape_layout(D, K, W, n)]
    Bp, wh, oH1, oH2, stride = lay[0], lay[3], lay[10], lay[11], lay[15]
    out = []
    for k in range(K):
        blk = tape[k * stride:(k + 1) * stride]
        out.append(tuple((blk[o:o + Bp * wh].view(Bp, wh)[:n, :W] > 0).cpu() for o in (oH1, oH2)))
    return out


@pytest.mark.parametrize("D,K,nodes,act_norm,n", [s + (B,) for s in sf.SAMPLE_GRAD_SHAPES] + [(32, 4, 10, False, RAGGED)])
def test_sampling_backward(D, K, nodes, act_norm, n):
    """`fabhip::realnvp_sample_tape`: d loss / d theta - L, U, log_S through W^-1 among them - and d loss / d eps of a loss in x and
    log q against float64 autograd through the oracle sampler (the loss of test_gpu_sample_grad.py), at (100, 1.0)."""
    c = case(D, K, nodes, 100.0, 1.0, act_norm, n)
    nf = c["nf"]
    hf = hip_flow(nf).requires_grad_(True)
    g = torch.Generator().manual_seed(5)
    a, cc, w = torch.randn(n, generator=g) / n, torch.randn(n, D, generator=g) / n, torch.rand(n, generator=g) / n
    loss_of = lambda x, lq, a, cc, w: (a * lq).sum() + (cc * x).sum() + 0.5 * (w[:, None] * x * x).sum()     # noqa: E731
    ed = c["eps"].to(DEV).requires_grad_(True)
    x_h, lq_h = hf.sample_and_log_prob((n,), eps=ed)
    assert x_h.requires_grad and lq_h.requires_grad
    dec = sample_tape_decisions(hf, x_h.detach())
    names = [k for k, _ in nf.named_parameters()]
    hp = dict(hf._nf_model.named_parameters())
    assert set(hp) == set(names)
    for p in hp.values():
        p.grad = None
    loss_of(x_h, lq_h, a.to(DEV), cc.to(DEV), w.to(DEV)).backward()
    torch.cuda.synchronize()
    ref = {}
    for dtype in (torch.float64, torch.float32):
        m = forced(nf, dec, dtype)
        e = c["eps"].to(dtype).requires_grad_(True)
        x, lq = m.sample_eps(e)
        loss_of(x, lq, a.to(dtype), cc.to(dtype), w.to(dtype)).backward()
        ref[dtype] = (x.detach(), lq.detach(), [p.grad for _, p in m.named_parameters()], e.grad)
    x64, l64, g64, ge64 = ref[torch.float64]
    x32, l32, g32, ge32 = ref[torch.float32]
    print(sf.row_rule("sample x", x_h.detach(), x32, x64)[1])
    print(sf.row_rule("sample log q", lq_h.detach(), l32, l64)[1])
    print(sf.row_rule("d loss / d eps", ed.grad, ge32, ge64)[1])
    judge_tensors(names, [hp[k].grad for k in names], g32, g64)
