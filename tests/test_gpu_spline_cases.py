"""The spline-flow kernels away from near-uniform bins (tests/spline_cases.py): bins from the minimum width to most of the range,
knot derivatives over both outer softplus branches, inputs on knots, on the tail bound and one ulp off it, end bins of the parameter
cotangents.  Yardstick: the float64 copy of the oracle flow; the fp32 oracle on the same inputs is the measure of what float32 can
do.  test_spline_cases.py holds the case list, the fp32 oracle and a second float32 evaluation to the same rules without a GPU.

RULES (spline_cases.band_rule).  A row passes by (i) `helpers.close`, (ii) an error <= 4x the fp32 oracle's on that row, (iii)
gradients: <= 4x the float64 spread under a 2.4e-7 relative input perturbation, at most n // 8 rows - or, on `knots` and `edges` rows,
by lying inside the float64 values of the 17 neighbours x (1 + k 6e-8); at most n // 8 rows of a continuous value (log q, y) may need
that width.  Where the fp32 oracle is inside a quarter of the tolerance (spline_cases.PLAIN) plain `close` is asserted.

Groups: (a) density and d log q / dx on every route, (b) samples and their log q, the round trip, (c) parameter gradients element by
element, (d) the sampling backward, (e) flows whose conditioner matters (the deep group).  Measured figures: tests/README.md."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

import spline_cases as sc
from helpers import close, worst, RTOL

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops            # noqa: E402

DEV = "cuda"
K = sc.K


def hip_from(of, D, L, H, circ, seed):
    """test_gpu_spline.make_pair's HIP half: the flow loaded from the oracle's state_dict."""
    hf = fa.CircularCoupledRQSFlow(D, L, H, circ, sc.tail_bounds(D, circ), seed=seed)
    res = hf._nf_model.load_state_dict(of.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return hf.to(DEV).requires_grad_(False)


@functools.lru_cache(maxsize=4)
def element_hip(fam, D, H, circ, L):
    of, _, seed = sc.element_flow(fam, D, H, circ, L)
    return hip_from(of, D, L, H, circ, seed)


@functools.lru_cache(maxsize=2)
def deep_hip(D, L, H, circ, level):
    of, _, seed = sc.deep_flow(D, L, H, circ, level)
    return hip_from(of, D, L, H, circ, seed)


def show(rep, tag):
    for r in rep:
        print(f"REPORT|{tag}|{r[0]}")


def same(a, b):
    """torch.equal that takes NaN for equal to NaN."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def tape_density(hf, xd):
    """log q and d log q / dx by autograd through log_prob with parameters that require grad: the staged pass with a tape."""
    hf.requires_grad_(True)
    try:
        xg = xd.clone().requires_grad_(True)
        lq = hf.log_prob(xg)
        assert lq.requires_grad
        (g,) = torch.autograd.grad(lq.sum(), xg)
    finally:
        hf.requires_grad_(False)
    return lq.detach(), g


def density_on(route, hf, xd, H):
    """(log q, d log q / dx) of one route.  The library does not report which kernel ran; the options select it (spline_stream.hip:
    r8_row_blocks, spline_log_prob_impl) and test_deep_group asserts, where the conditioner's sums matter, that the 16x16x4 and the
    stream kernel do not return the same bits."""
    if route == "default":
        lq, g = hf.log_prob_and_grad(xd)
        assert same(hf.log_prob(xd), lq), "density-only and density + gradient launches disagree"
        return lq, g
    if route == "mfma16":
        assert H > 128
        with _ops.option(_ops.OPT_SPLINE_MFMA, 16):
            return hf.log_prob_and_grad(xd)
    if route == "stream":
        assert H > 128
        out = []
        for shape in (4, 8, 16):
            with _ops.option(_ops.OPT_TILE_SHAPE, shape):
                out.append(hf.log_prob_and_grad(xd))
        for lq, g in out[1:]:
            assert same(lq, out[0][0]) and same(g, out[0][1]), "the tile shapes of the stream kernel differ"
        return out[0]
    if route == "staged":
        with _ops.option(_ops.OPT_SPLINE_STAGED, 1):
            return hf.log_prob_and_grad(xd)
    assert route == "tape"
    return tape_density(hf, xd)


def routes_of(H):
    return ["default", "staged", "tape"] + (["mfma16", "stream"] if H > 128 else [])


def _a_cases():
    return [c + (r,) for c in sc.ELEMENT_CASES for r in routes_of(c[2])]


# ---- (a) density and gradient on every route ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,D,H,circ,L,route", _a_cases())
def test_density_and_gradient(fam, D, H, circ, L, route):
    hf = element_hip(fam, D, H, circ, L)
    for grp, n in [(g, None) for g in sc.GROUPS] + list(sc.RAGGED.items()):
        c = sc.density_case(fam, D, H, circ, L, grp, n)
        lq, g = density_on(route, hf, c["x"].to(DEV), H)
        keep_g = not sc.hip_dropped("gradient", fam, D, L, grp if n is None else f"{grp}{n}")
        show(sc.check_density(c, lq.cpu(), g.cpu(), grp, fam, gradient=keep_g), f"a|{fam}|{route}|D={D} L={L}" + ("" if n is None else f" n={n}"))


@pytest.mark.parametrize("fam,D,H,circ,L", sc.ELEMENT_CASES)
def test_special_rows(fam, D, H, circ, L):
    """A NaN, +inf or -inf coordinate: log q is NaN / -inf exactly where the oracle has them, nothing is raised, and every other row
    of the batch is bit-identical to the same batch without them."""
    hf = element_hip(fam, D, H, circ, L)
    of, of64, _ = sc.element_flow(fam, D, H, circ, L)
    dens, _ = sc.probe_rows(of64)
    x, sp = dens["special"], dens["special_rows"]
    with torch.no_grad():
        l32 = of.log_prob(x)
    n0 = len(dens["interior"])
    for route in routes_of(H):
        lq, g = density_on(route, hf, x.to(DEV), H)
        lq0, g0 = density_on(route, hf, x[:n0].contiguous().to(DEV), H)
        torch.cuda.synchronize()
        lq = lq.cpu()
        assert torch.equal(lq[:n0], lq0.cpu()) and torch.equal(g[:n0].cpu(), g0.cpu()), f"{route}: a special row changed another row"
        pat = lambda t: ["nan" if math.isnan(v) else ("-inf" if v == -math.inf else ("+inf" if v == math.inf else "finite"))  # noqa: E731
                         for v in t[sp].tolist()]
        assert pat(lq) == pat(l32), f"{route}: special rows give {pat(lq)}, the oracle {pat(l32)}"
        assert bool(torch.isfinite(lq[:n0]).all())


# ---- (b) samples ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,D,H,circ,L", sc.ELEMENT_CASES)
def test_samples_and_round_trip(fam, D, H, circ, L):
    hf = element_hip(fam, D, H, circ, L)
    of = sc.element_flow(fam, D, H, circ, L)[0]
    for grp, n in [(g, None) for g in sc.GROUPS] + list(sc.RAGGED.items()):
        if sc.hip_dropped("sample", fam, D, L, grp if n is None else f"{grp}{n}") or sc.hip_dropped("sample", fam, D, L, grp):
            continue
        c = sc.sample_case(fam, D, H, circ, L, grp, n)
        x, ls = hf.sample_and_log_prob((len(c["u"]),), u=c["u"].to(DEV), eps=c["eps"].to(DEV))
        tag = f"b|{fam}|sample|D={D} L={L}" + ("" if n is None else f" n={n}")
        show(sc.check_sample(c, x.cpu(), ls.cpu(), grp, fam), tag)
        if sc.hip_dropped("round trip", fam, D, L, grp if n is None else f"{grp}{n}"):
            continue
        # round trip: log_prob of the kernel's own samples against the sampling log q (float64's), the oracle's own round trip as o32
        rt = hf.log_prob(x).cpu()
        with torch.no_grad():
            rt32 = of.log_prob(c["x32"])
        for rows in sc.split_far(c["eps"]) if grp == "edges" else [np.arange(len(c["eps"]))]:
            band = tuple(t[rows] for t in c["band_ls"]) if grp in ("knots", "edges") else None
            show([sc.band_rule(f"round trip {grp} log q", rt[rows], rt32[rows], c["ls64"][rows], band, continuous=True)], tag)


# ---- (c) parameter gradients, element by element ---------------------------------------------------------------------------------------------
def elementwise(name, hip, o32, f64, tag):
    """A [n, 8 | 9 | 25] gradient (one row per coordinate) element by element: rule (i) or (ii), scale = the tensor's largest entry."""
    s = float(f64.abs().max())
    if s == 0.0:
        assert not bool(hip.any()), f"{name}: float64 is exactly zero, HIP is not"
        return
    show([sc.plain_rule(name, hip.double() / s, o32.double() / s, f64 / s)], tag)


def by_norm(name, hip, o32, f64):
    """test_gpu_spline.test_spline_flow_parameter_gradients_vs_oracle's bound: relative L2 against float64 within max(1e-4, 3x the
    fp32 oracle's)."""
    n64 = float(f64.norm())
    if n64 == 0.0:
        assert not bool(hip.any()), f"{name}: float64 is exactly zero, HIP is not"
        return
    eh, eo = float((hip.double() - f64).norm()) / n64, float((o32.double() - f64).norm()) / n64
    assert eh <= max(1e-4, 3.0 * eo), f"{name}: HIP {eh:.2e} from float64 (fp32 CPU oracle {eo:.2e})"


def compare_param_grads(hf, g32, g64, tag):
    for name, p in hf._nf_model.named_parameters():
        assert p.grad is not None, name
        h = p.grad.cpu()
        if name.endswith("final_layer.bias"):
            elementwise(name, h.view(-1, sc.NP), g32[name].view(-1, sc.NP), g64[name].view(-1, sc.NP), tag)
        elif "unconditional_transform" in name:
            elementwise(name, h, g32[name], g64[name], tag)
        else:
            by_norm(name, h, g32[name], g64[name])


def oracle_param_grads(of, of64, loss):
    """{name: gradient} of `loss(flow, dtype)` for copies of the fp32 oracle and of its float64 twin (the cached flows stay as they are)."""
    out = []
    for f, dt in ((copy.deepcopy(of), torch.float32), (copy.deepcopy(of64), torch.float64)):
        loss(f, dt).backward()
        out.append({n: p.grad.detach().clone() for n, p in f.named_parameters()})
    return out


@pytest.mark.parametrize("fam,D,H,circ,L", [c for c in sc.ELEMENT_CASES if not sc.hip_dropped("parameter gradients", c[0], c[1], c[4])])
def test_parameter_gradients_element_by_element(fam, D, H, circ, L):
    """d (sum_b c_b log q(x_b)) / d theta.  With the final weight zero d / d final_layer.bias is the batch sum of rqs_backward's 25
    cotangents per transformed coordinate, the unconditional tensors give the identity coordinates': compared entry by entry, on
    rows of all bins and on batches that sit in bin 0 / bin K - 1 only (the fixed end knots W_0, W_K and, on linear coordinates, the
    fixed end derivatives)."""
    of, of64, _ = sc.element_flow(fam, D, H, circ, L)
    hf = element_hip(fam, D, H, circ, L)
    for grp in ("interior", "bin0", "binK"):
        c = sc.density_case(fam, D, H, circ, L, grp)
        x = c["x"]
        cb = torch.randn(len(x), generator=torch.Generator().manual_seed(len(x) + D))
        g32, g64 = oracle_param_grads(of, of64, lambda f, dt: (cb.to(dt) * f.log_prob(x.to(dt))).sum())
        hf.requires_grad_(True)
        try:
            for p in hf.parameters():
                p.grad = None
            (cb.to(DEV) * hf.log_prob(x.to(DEV))).sum().backward()
            compare_param_grads(hf, g32, g64, f"c|{fam}|{grp}|D={D} L={L}")
        finally:
            hf.requires_grad_(False)
            for p in hf.parameters():
                p.grad = None


# ---- (d) the sampling backward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,D,H,circ,L,grp", [c + (g,) for c in sc.ELEMENT_CASES if c[0] in ("E1", "E2")
                                                for g in ("interior", "bin0", "binK")
                                                if not sc.hip_dropped("sampling backward", c[0], c[1], c[4], g)])
def test_sampling_backward(fam, D, H, circ, L, grp):
    """spline_sample_vjp_tape: d (sum_b c_b log q_b + sum r_bj x_bj) / d (theta, u, eps) on draws that visit every height bin, and on
    batches whose draws all sit in the first / the last height bin."""
    of, of64, _ = sc.element_flow(fam, D, H, circ, L)
    hf = element_hip(fam, D, H, circ, L)
    c = sc.sample_case(fam, D, H, circ, L, grp)
    n = len(c["u"])
    gen = torch.Generator().manual_seed(3 + D)
    cb, r = torch.randn(n, generator=gen), torch.randn(n, D, generator=gen)
    noise = {}

    def loss(f, dt):
        u, eps = c["u"].clone().to(dt).requires_grad_(True), c["eps"].clone().to(dt).requires_grad_(True)
        noise[dt] = (u, eps)
        x, lq = f.sample_eps(u, eps)
        return (cb.to(dt) * lq).sum() + (r.to(dt) * x).sum()
    g32, g64 = oracle_param_grads(of, of64, loss)
    hf.requires_grad_(True)
    try:
        for p in hf.parameters():
            p.grad = None
        u, eps = c["u"].clone().to(DEV).requires_grad_(True), c["eps"].clone().to(DEV).requires_grad_(True)
        x, lq = hf.sample_and_log_prob((n,), u=u, eps=eps)
        ((cb.to(DEV) * lq).sum() + (r.to(DEV) * x).sum()).backward()
        tag = f"d|{fam}|{grp}|D={D} L={L}"
        compare_param_grads(hf, g32, g64, tag)
        circ_mask = of.q0.circ
        for name, h, i in (("d / du", u.grad.cpu(), 0), ("d / d eps", eps.grad.cpu(), 1)):
            o32, f64 = noise[torch.float32][i].grad, noise[torch.float64][i].grad
            cols = circ_mask if i == 0 else ~circ_mask
            assert not bool(h[:, ~cols].any()), f"{name}: a gradient on a coordinate whose base draw does not use it"
            if bool(cols.any()):
                show([sc.plain_rule(name, h[:, cols], o32[:, cols], f64[:, cols])], tag)
    finally:
        hf.requires_grad_(False)
        for p in hf.parameters():
            p.grad = None


# ---- (e) the deep group ----------------------------------------------------------------------------------------------------------------------
def _e_cases():
    out = []
    for (D, L, H, circ) in sc.DEEP_SHAPES:
        for lv in sc.DEEP_LEVELS:
            if (D, L, H, circ, lv) in sc.DEEP_DROPPED or sc.hip_dropped("deep", lv, D, L):
                continue
            out.append((D, L, H, circ, lv, sc.DEEP_B))
            if (D, lv) == (12, sc.DEEP_LEVELS[0]):
                out.append((D, L, H, circ, lv, sc.DEEP_RAGGED))
    return out


@pytest.mark.parametrize("D,L,H,circ,level,n", _e_cases())
def test_deep_group(D, L, H, circ, level, n):
    c = sc.deep_case(D, L, H, circ, level, n)
    hf = deep_hip(D, L, H, circ, level)
    tag = f"e|deep {level}|default|D={D} L={L} H={H} n={n}"
    xd = c["x"].to(DEV)
    lq, g = density_on("default", hf, xd, H)
    show(sc.check_density(c, lq.cpu(), g.cpu(), "deep"), tag)
    x, ls = hf.sample_and_log_prob((n,), u=c["u"].to(DEV), eps=c["eps"].to(DEV))
    show(sc.check_sample(c, x.cpu(), ls.cpu(), "deep"), tag)
    if H > 128:
        lq16, g16 = density_on("mfma16", hf, xd, H)
        assert not torch.equal(lq16, lq), "the 16x16x4 and the stream route returned the same bits: one kernel ran twice"
        show(sc.check_density(c, lq16.cpu(), g16.cpu(), "deep"), tag.replace("default", "mfma16"))
        lqs, gs = density_on("stream", hf, xd, H)
        assert torch.equal(lqs, lq) and torch.equal(gs, g), "the default launch at hidden 256 is not the stream kernel"


@pytest.mark.parametrize("D,L,H,circ,level,n", [c for c in _e_cases() if c[5] == sc.DEEP_B])
def test_deep_group_parameter_gradients(D, L, H, circ, level, n):
    c = sc.deep_case(D, L, H, circ, level, n)
    hf = deep_hip(D, L, H, circ, level)
    cb = torch.randn(n, generator=torch.Generator().manual_seed(n + D))
    x = c["x"]
    g32, g64 = oracle_param_grads(c["of"], c["of64"], lambda f, dt: (cb.to(dt) * f.log_prob(x.to(dt))).sum())
    hf.requires_grad_(True)
    try:
        for p in hf.parameters():
            p.grad = None
        (cb.to(DEV) * hf.log_prob(x.to(DEV))).sum().backward()
        for name, p in hf._nf_model.named_parameters():
            by_norm(name, p.grad.cpu(), g32[name], g64[name])
    finally:
        hf.requires_grad_(False)
        for p in hf.parameters():
            p.grad = None
