"""RQ-spline coupling flows away from near-uniform bins (shared by test_spline_cases.py and test_gpu_spline_cases.py).

`oracle.spline.randomize(std <= 0.4)` leaves every conditional spline within a few percent of uniform bins and its knot
derivatives in 0.8 .. 1.3: the outer branches of the softplus, a bin at the minimum width, a slope h / w far from 1, the end bins
of the parameter cotangents and an input exactly on a knot are never reached.  `set_spline` re-draws the parameters that decide
them; `probe_rows` puts rows where the element functions branch; `band_rule` is how a row that sits on a knot is judged.

ELEMENT FAMILIES (final-layer weight zero: the conditional spline's parameters are its bias, its knots are known in float64):
  E1 logits N(0, 1),   derivative logits from (-1, 0, .54, 1.5, 3)             - uneven bins, moderate slopes
  E2 logits N(0, 0.3), derivative logits over both outer softplus branches     - even bins, knot derivatives 1e-3 .. 25
  E3 logits N(0, 3),   derivative logits as E1                                 - bins from the minimum width to > 0.8 of the range
Extreme bins AND extreme derivatives together are left out on purpose: beside a knot with derivative 1e-3 next to a bin of
slope 900 log|dy/dx| moves by 4.5 over the float32 rounding of the knot position - no float32 implementation matches float64.

RULES.  `stressed_flow.row_rule`: (i) helpers.close, (ii) error <= 4x the fp32 oracle's on the row, (iii) gradients: <= 4x the
float64 spread under a 2.4e-7 relative input perturbation.  `knots` and `edges` rows add the NEIGHBOURHOOD rule: the value lies,
element-wise, within [min - tol, max + tol] of the float64 values at x (1 + k 6e-8), k = -8 .. 8 (d log q / dx is discontinuous at
a knot, and the float32 knot is not the float64 knot: the bin of such a row may differ by one).  It asks neither implementation.
Caps: at most n // 8 rows of a comparison by (iii) only; at most n // 8 rows of a `knots` comparison of a CONTINUOUS value (log q,
y) may pass through the neighbourhood's width alone."""
import copy
import functools
import math

import numpy as np
import torch

import stressed_flow as sf
from helpers import RTOL
from oracle import spline as osp

K = 8
NP = 3 * K + 1
NB_STEP, NB_K = 6e-8, 8
UD_E1 = (-1.0, 0.0, 0.54, 1.5, 3.0)
UD_E2 = (-30.0, -9.0, -5.001, -4.999, -1.0, 0.54, 3.0, 19.999, 20.001, 25.0)
FAMILIES = {"E1": (1.0, UD_E1), "E2": (0.3, UD_E2), "E3": (3.0, UD_E1)}
# (D, hidden, circular coordinates): D = 2 is the smallest shape check_spline_shape admits; hidden 128 is the NTWM = 2 variant
E_SHAPES = [(2, 16, ()), (6, 64, (1, 4)), (8, 256, (0, 7)), (7, 128, (0, 6))]
E_SHAPES_L2 = [(6, 64, (1, 4)), (8, 256, (0, 7))]          # L <= 2 has no PeriodicShift
ELEMENT_CASES = [(fam, D, H, circ, 1) for fam in FAMILIES for (D, H, circ) in E_SHAPES] \
    + [(fam, D, H, circ, 2) for fam in FAMILIES for (D, H, circ) in E_SHAPES_L2]
# seed of a case where the default (below) misses the branch coverage test_spline_cases.py asserts (E2: every outer softplus branch
# and both thresholds on an effective knot; E3: a bin at the minimum width and one above 0.8 of the range).  From the float64
# parameters alone.
SEED_OVERRIDE = {("E3", 2, 16, (), 1): 252, ("E3", 6, 64, (1, 4), 1): 202, ("E3", 8, 256, (0, 7), 1): 200,
                 ("E3", 7, 128, (0, 6), 1): 201, ("E3", 6, 64, (1, 4), 2): 200}
GROUPS = ("interior", "knots", "edges", "bin0", "binK")
RAGGED = {"interior": 37, "edges": 1}                     # the 37 rows: five per bin (the three of `interior` + 25 % and 75 %)

DEEP_SHAPES = [(8, 4, 64, (1, 4, 6)), (12, 3, 200, (2, 5)), (32, 6, 256, ()), (60, 4, 256, (3, 7, 30, 59))]
DEEP_LEVELS = [(0.25, 0.5), (0.5, 1.0)]                    # (logit std after the sqrt(hidden) division, derivative-logit std)
DEEP_B, DEEP_RAGGED = 64, 37
DEEP_MAX_GRAD = 1e5
# (D, L, hidden, circ, level) on which one of three permuted twins of the fp32 oracle leaves the rule (test_spline_cases.py prints
# the row); never a GPU result
DEEP_DROPPED = {(12, 3, 200, (2, 5), (0.5, 1.0)), (32, 6, 256, (), (0.5, 1.0)), (60, 4, 256, (3, 7, 30, 59), (0.5, 1.0))}
# (family, group, quantity) on which test_spline_cases.py finds the fp32 oracle inside a quarter of the tolerance on every shape:
# the GPU file asserts plain `close` there, no clause.  quantity: "lq" (density), "x" / "ls" (sample and its log q).  Groups with
# a neighbourhood (`knots`, `edges`) are not listed: their rows sit on a discontinuity (a knot of d log q / dx; +-tb, where the
# next layer takes the identity branch for an input one ulp outside), where the oracle's own agreement with float64 is a coin flip.
PLAIN = {("E1", g, q) for g, q in (("bin0", "lq"), ("bin0", "x"), ("bin0", "ls"), ("binK", "lq"), ("binK", "ls"), ("interior", "x"))} \
    | {("E2", g, q) for g, q in (("bin0", "lq"), ("bin0", "x"), ("bin0", "ls"), ("binK", "lq"), ("binK", "x"), ("binK", "ls"),
                                 ("interior", "lq"), ("interior", "x"))}
# Comparisons of test_gpu_spline_cases.py left out because HIP leaves the rule there by conditioning, not by a defect (the figures:
# tests/README.md, "Spline flow away from near-uniform bins"): (what, family, D, L, group), None = every.
HIP_DROPPED = {
    # y on a height knot whose derivative is 1e-3: the inverse's discriminant is the difference of two terms 4e6 times larger
    ("sample", "E2", None, None, "knots"), ("round trip", "E2", 6, 2, "interior37"),
    # a sample that went through bins of slope 1e-3 .. 1e3: the fp32 oracle's own x is up to 5e3 units off, its log q up to 9e2
    ("sample", "E3", None, None, None),
    # 4 (cap 3) and 5 (cap 4) rows of the gradient need clause (iii), one row at 2.0 units passes none; the fp32 oracle alone needs
    # (iii) on 15 of 24
    ("gradient", "E3", 2, 1, "interior"), ("gradient", "E3", 2, 1, "interior37"), ("gradient", "E3", 6, 1, "interior37"),
    ("parameter gradients", "E3", 6, 1, None), ("parameter gradients", "E3", 8, 1, None), ("parameter gradients", "E3", 7, 1, None),
    ("parameter gradients", "E1", 6, 2, None), ("parameter gradients", "E2", 6, 2, None),
    ("sampling backward", "E2", 6, 2, None), ("sampling backward", "E2", 8, 2, None), ("sampling backward", "E1", 6, 2, "binK"),
    # the deep group: one row of log q at 1.0 units where the fp32 oracle is at 0.1
    ("deep", (0.5, 1.0), 8, 4, None),
}


def hip_dropped(what, fam, D, L, group=None):
    return any(k in HIP_DROPPED for k in ((what, fam, D, L, group), (what, fam, D, L, None), (what, fam, None, None, group),
                                          (what, fam, None, None, None)))


def case_seed(fam, D, H, circ, L):
    return SEED_OVERRIDE.get((fam, D, H, tuple(circ), L), 40 + 3 * D + L + 7 * list(FAMILIES).index(fam))


def tail_bounds(D, circ):
    """5 on the linear coordinates; float32(pi) and pi / 0.8 alternate on the circular ones."""
    tb = torch.full((D,), 5.0)
    for n, c in enumerate(circ):
        tb[c] = math.pi if n % 2 == 0 else math.pi / 0.8
    return tb


def couplings(nf):
    return [f for f in nf.flows if isinstance(f, osp.CircularCoupledRationalQuadraticSpline)]


def _draw_list(values, n, g):
    """[n, K + 1] entries of `values`: a shuffled tiling, so that every value appears as often as any other."""
    v = torch.tensor(values)
    idx = torch.arange(n * (K + 1)) % len(values)
    return v[idx[torch.randperm(n * (K + 1), generator=g)]].view(n, K + 1)


def set_spline(of, logit_std, ud_values=None, ud_std=None, weight_scale=0.0, seed=0):
    """Re-draw, for every coupling layer of the oracle flow `of`, in place: the final-layer bias (width / height logits
    N(0, logit_std) sqrt(hidden) - the flow divides them by sqrt(hidden) -, derivative logits from the list `ud_values` or
    0.54 + N(0, ud_std)), the final-layer weight (zero, or `weight_scale` N(0, 0.6 std / sqrt(hidden)) with std that of the
    output's bias; then also the block's second Linear as `randomize` has it, so that the hidden units matter), the unconditional
    widths / heights / derivatives at the same scales, the periodic-feature weights as `randomize` does."""
    assert (ud_values is None) != (ud_std is None)
    g = torch.Generator().manual_seed(int(seed))
    r = lambda *s: torch.randn(*s, generator=g)               # noqa: E731
    with torch.no_grad():
        for f in couplings(of):
            net, u = f.prqct.transform_net, f.prqct.unconditional_transform
            H, nt, ni = net.hidden_features, len(f.prqct.transform_features), len(f.prqct.identity_features)
            p = torch.zeros(nt, NP)
            p[:, :2 * K] = r(nt, 2 * K) * logit_std * math.sqrt(H)
            p[:, 2 * K:] = _draw_list(ud_values, nt, g) if ud_values is not None else 0.54 + r(nt, K + 1) * ud_std
            net.final_layer.bias.copy_(p.reshape(-1))
            if weight_scale:
                std = torch.ones(nt, NP)
                std[:, :2 * K] = logit_std * math.sqrt(H)
                std[:, 2 * K:] = ud_std if ud_std is not None else 1.0
                net.final_layer.weight.copy_(r(nt * NP, H) * std.reshape(-1, 1) * (0.6 * weight_scale / math.sqrt(H)))
                lin = net.blocks[0].linear_layers[1]
                lin.weight.copy_(r(*lin.weight.shape) * 0.05)
            else:
                net.final_layer.weight.zero_()
            u.unnormalized_widths.copy_(r(ni, K) * logit_std)
            u.unnormalized_heights.copy_(r(ni, K) * logit_std)
            u.unnormalized_derivatives.copy_(_draw_list(ud_values, ni, g) if ud_values is not None
                                             else 0.54 + r(ni, K + 1) * ud_std)
            if net.preprocessing is not None:
                net.preprocessing.weights.add_(r(*net.preprocessing.weights.shape) * 0.2)


def make_flow(D, L, H, circ, seed):
    torch.manual_seed(seed)                                   # nn.Linear's default init draws from the global generator
    return osp.make_circular_coupled_flow(D, L, H, circ, tail_bounds(D, circ), seed=seed)


@functools.lru_cache(maxsize=None)
def element_flow(fam, D, H, circ, L):
    """(fp32 oracle flow, its float64 copy, flow seed) of an element case; never modified."""
    seed = case_seed(fam, D, H, circ, L)
    of = make_flow(D, L, H, circ, seed)
    logit_std, ud = FAMILIES[fam]
    set_spline(of, logit_std, ud_values=ud, seed=seed + 1)
    return of, copy.deepcopy(of).double(), seed


@functools.lru_cache(maxsize=None)
def deep_flow(D, L, H, circ, level):
    seed = 11 * D + L
    of = make_flow(D, L, H, circ, seed)
    set_spline(of, level[0], ud_std=level[1], weight_scale=1.0, seed=seed + 1)
    return of, copy.deepcopy(of).double(), seed


def permuted_twin(of, seed=0):
    """The same function in another summation order: the hidden units of every ResidualNet permuted consistently (rows of the
    initial layer and of the block Linears, columns of the block Linears and of the final layer)."""
    tw = copy.deepcopy(of)
    g = torch.Generator().manual_seed(500 + int(seed))
    with torch.no_grad():
        for f in couplings(tw):
            net = f.prqct.transform_net
            pm = torch.randperm(net.hidden_features, generator=g)
            net.initial_layer.weight.copy_(net.initial_layer.weight[pm].clone())
            net.initial_layer.bias.copy_(net.initial_layer.bias[pm].clone())
            for lin in net.blocks[0].linear_layers:
                lin.weight.copy_(lin.weight[pm][:, pm].clone())
                lin.bias.copy_(lin.bias[pm].clone())
            net.final_layer.weight.copy_(net.final_layer.weight[:, pm].clone())
    return tw


# ---- the knots of a layer whose final weight is zero ---------------------------------------------------------------------------------
def cum_knots(u, tb):
    """oracle.spline.rational_quadratic_spline's knot positions of logits u [n, K] on [-tb, tb], in u's dtype: [n, K + 1]."""
    w = torch.softmax(u, -1)
    w = osp.MIN_BIN_WIDTH + (1 - osp.MIN_BIN_WIDTH * K) * w
    c = torch.nn.functional.pad(torch.cumsum(w, -1), (1, 0), value=0.0)
    c = (2 * tb)[:, None] * c - tb[:, None]
    c[:, 0] = -tb
    c[:, -1] = tb
    return c


def layer_params(f):
    """(uw, uh, ud) [D, K | K | K + 1] of every coordinate of coupling layer `f` (final weight zero) as the spline receives them:
    conditional logits divided by sqrt(hidden), end derivatives fixed (linear) or tied (circular)."""
    pr = f.prqct
    net, u = pr.transform_net, pr.unconditional_transform
    assert not bool(net.final_layer.weight.any())
    D = len(pr.identity_features) + len(pr.transform_features)
    p = net.final_layer.bias.detach().view(-1, NP)
    s = math.sqrt(net.hidden_features)
    out = torch.zeros(D, NP, dtype=p.dtype)
    out[pr.transform_features] = torch.cat([p[:, :2 * K] / s, p[:, 2 * K:]], 1)
    out[pr.identity_features] = torch.cat([u.unnormalized_widths, u.unnormalized_heights, u.unnormalized_derivatives], 1).detach()
    circ = torch.zeros(D, dtype=torch.bool)
    circ[pr.transform_features] = pr.circ_t
    circ[pr.identity_features] = u.circ
    ud = out[:, 2 * K:].clone()
    const = math.log(math.exp(1 - osp.MIN_DERIVATIVE) - 1)
    ud[~circ, 0] = const
    ud[~circ, -1] = const
    ud[circ, -1] = ud[circ, 0]
    return out[:, :K], out[:, K:2 * K], ud, circ


def layer_knots(f, tb, which):
    uw, uh, _, _ = layer_params(f)
    return cum_knots(uw if which == "w" else uh, tb.to(uw.dtype))


def bins_of(knots, x):
    """bin index [n, D] of x [n, D] among knots [D, K + 1] (x inside the range)."""
    return (x[:, :, None] >= knots[None, :, 1:K]).sum(-1)


def wrap(x, tb, circ):
    """PeriodicWrap.inverse in x's dtype."""
    x = x.clone()
    b = tb[circ].to(x.dtype)
    x[:, circ] = torch.remainder(x[:, circ] + b, 2 * b) - b
    return x


def coverage(fam, of64):
    """Which branches the float64 parameters of an element case reach, on the layer each direction probes: dict of bools, all of
    which test_spline_cases.py asserts (E2: an effective knot on each outer softplus branch and within 1e-3 (+ float32 rounding) of
    both thresholds; E3: a bin within 1 % of the minimum and one above 0.8 of the range)."""
    tb, _ = flow_meta(of64)
    out = {}
    for name, f, which in (("density", first_density_layer(of64), "w"), ("sample", first_sample_layer(of64), "h")):
        _, _, ud, _ = layer_params(f)
        kn = layer_knots(f, tb, which)
        frac = (kn[:, 1:] - kn[:, :-1]) / (2 * tb[:, None])
        if fam == "E2":
            out[name + ": ud > 20"] = bool((ud > 20).any())
            out[name + ": ud < -5"] = bool((ud < -5).any())
            out[name + ": ud just above 20"] = bool(((ud > 20) & (ud < 20.0011)).any())
            out[name + ": ud just below 20"] = bool(((ud < 20) & (ud > 19.9989)).any())
            out[name + ": ud just above -5"] = bool(((ud > -5) & (ud < -4.9989)).any())
            out[name + ": ud just below -5"] = bool(((ud < -5) & (ud > -5.0011)).any())
        if fam == "E3":
            out[name + ": a bin at the minimum"] = bool((frac <= 1.01 * osp.MIN_BIN_WIDTH).any())
            out[name + ": a bin above 0.8"] = bool((frac > 0.8).any())
    return out


# ---- probe rows ----------------------------------------------------------------------------------------------------------------------
def _f32(rows):
    return torch.stack(rows).float()


def _near(x, up):
    return torch.nextafter(x, torch.full_like(x, math.inf if up else -math.inf))


def probe_values(kn, tb, circ):
    """float32 rows [n, D], in named groups, from the float64 knots `kn` [D, K + 1] of one direction of a layer (width knots:
    points x of the density direction; height knots: base draws z of the sampling direction)."""
    D = kn.shape[0]
    lo, hi = kn[:, :-1], kn[:, 1:]
    at = lambda b, fr: lo[:, b] + fr * (hi[:, b] - lo[:, b])   # noqa: E731
    out = {"interior": _f32([at(b, fr) for b in range(K) for fr in (0.03, 0.5, 0.97)]),
           "interior37": _f32([at(b, fr) for b in range(K) for fr in (0.03, 0.25, 0.5, 0.75, 0.97)])[:37]}
    xk = _f32([kn[:, j] for j in range(1, K)])
    out["knots"] = torch.cat([xk, _near(xk, True), _near(xk, False)])
    fr8 = (0.02, 0.15, 0.3, 0.45, 0.6, 0.75, 0.9, 0.98)
    out["bin0"] = _f32([at(0, fr) for fr in fr8])
    out["binK"] = _f32([at(K - 1, fr) for fr in fr8])
    t = tb.float()
    z = torch.zeros(D)
    rows = [t, -t, _near(t, False), _near(t, True), _near(-t, True), _near(-t, False), z + 7.0, z + 1e4, z, -z]
    if circ.any():
        base = 0.3 * torch.ones(D)
        for v in (math.pi, -math.pi, 3 * math.pi, -5 * math.pi + 0.1):
            r = base.clone()
            r[circ] = v
            rows.append(r)
    out["edges"] = torch.stack(rows).float()
    # special: an interior batch whose last rows carry one NaN / +inf / -inf coordinate, on a linear and on a circular coordinate
    sp, where = [], []
    lin = [j for j in range(D) if not bool(circ[j])]
    cc = [j for j in range(D) if bool(circ[j])]
    for j in ([lin[0]] if lin else []) + ([cc[0]] if cc else []):
        for n, v in enumerate((math.nan, math.inf, -math.inf)):
            r = out["interior"][3 * n + 1].clone()
            r[j] = v
            sp.append(r)
            where.append(j)
    out["special"] = torch.cat([out["interior"], torch.stack(sp)])
    out["special_rows"] = list(range(len(out["interior"]), len(out["special"])))
    return out


def first_density_layer(nf):
    return couplings(nf)[-1]


def first_sample_layer(nf):
    return couplings(nf)[0]


def flow_meta(nf):
    D = nf.q0.circ.shape[0]
    f = couplings(nf)[0].prqct
    tb = torch.zeros(D, dtype=torch.float64)
    tb[f.transform_features] = f.tb_t.double()
    tb[f.identity_features] = f.unconditional_transform.tail_bound.double()
    return tb, nf.q0.circ.clone()


def probe_rows(of64):
    """(density rows, sampling draws): dicts group -> float32 tensors.  Density rows are points x on the width knots of the first
    layer log_prob meets; sampling draws are (u, eps) whose base draw z = (u - 0.5) 2 tb (circular) / eps (linear) lands on the height
    knots of the first layer the sampler meets."""
    tb, circ = flow_meta(of64)
    dens = probe_values(layer_knots(first_density_layer(of64), tb, "w"), tb, circ)
    zs = probe_values(layer_knots(first_sample_layer(of64), tb, "h"), tb, circ)
    samp = {}
    scale = of64.q0.scale.float()
    for k, z in zs.items():
        if k in ("special", "special_rows"):
            continue
        if k == "edges":                                       # the base draw of a circular coordinate cannot leave [-tb, tb]
            z = z[:10].clone()
            z[6:8, circ] = 0.25 * tb[circ].float()
        v = z / scale                                          # u - 0.5
        u = torch.where(circ, v + 0.5, torch.full_like(z, 0.5)).clamp(0.0, 1.0)
        eps = torch.where(circ, torch.zeros_like(z), z)
        samp[k] = (u, eps)
    return dens, samp


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------
logq_grad = sf.logq_grad


def sample(nf, u, eps):
    with torch.no_grad():
        return nf.sample_eps(u, eps)


def nb_band(fn, *args):
    """[(lo, hi)] per output of fn: element-wise extremes of the float64 fn over its arguments scaled by 1 + k 6e-8, k = -8 .. 8."""
    outs = [fn(*[a.double() * (1 + k * NB_STEP) for a in args]) for k in range(-NB_K, NB_K + 1)]
    bands = []
    for i in range(len(outs[0])):
        v = torch.stack([o[i].detach() for o in outs])
        bands.append((v.amin(0), v.amax(0)))
    return bands


def density_band(of64, x):
    return nb_band(lambda xx: logq_grad(of64, xx), x)


def sample_band(of64, u, eps):
    return nb_band(lambda v, e: sample(of64, v + 0.5, e), u.double() - 0.5, eps)


def row_errs(a, f64):
    """`stressed_flow.row_errors` where a row of `a` may be non-finite (float64 is finite): such a row has error inf."""
    an, fn = sf._np(a), sf._np(f64)
    assert np.isfinite(fn).all(), "float64 is not finite"
    bad = ~np.isfinite(an.reshape(len(an), -1)).all(1)
    an = an.copy()
    an[bad] = fn[bad]
    e, u = sf.row_errors(an, fn)
    e[bad], u[bad] = np.inf, np.inf
    return e, u


def band_units(a, lo, hi, scale):
    """per row: how far `a` lies outside [lo, hi], in units of the tolerance of helpers.close (<= 1: inside the widened band)."""
    a, lo, hi = (sf._np(t).reshape(len(lo), -1) for t in (a, lo, hi))
    tol = RTOL * np.maximum(np.abs(lo), np.abs(hi)) + 2e-6 * scale
    with np.errstate(invalid="ignore"):
        return np.nan_to_num((np.maximum(np.maximum(lo - a, a - hi), 0.0) / tol).max(1), nan=np.inf)


def band_rule(what, a, o32, f64, band, continuous, spread=None):
    """The row rule, with the neighbourhood clause where `band` = (lo, hi) is given.  Returns (message, worst units of `a`, of
    `o32`, rows beyond (i), rows by (iii) only, rows that pass by the neighbourhood's width alone); raises on a row that passes no
    clause and on a broken cap.  A non-finite row of `a` (float64 finite) has error inf and passes no clause, also where the fp32
    oracle's row is non-finite (such a row of the ORACLE has error inf: clause (ii) then takes any finite value)."""
    n = len(f64)
    eh, uh = row_errs(a, f64)
    eo, uo = row_errs(o32, f64)
    scale = max(1.0, float(np.abs(sf._np(f64)).max()))
    inside = band_units(a, band[0], band[1], scale) <= 1.0 if band is not None else np.zeros(n, dtype=bool)
    ok12 = ((uh <= 1.0) | (eh <= 4 * eo)) & np.isfinite(eh)   # (a non-finite row of `a` passes nothing, whatever the oracle has)
    only3 = np.zeros(n, dtype=bool)
    if spread is not None and not (ok12 | inside).all():
        rows = np.nonzero(~(ok12 | inside))[0]
        only3[rows] = eh[rows] <= 4 * np.asarray(spread(rows))
    width = ~ok12 & inside
    msg = (f"{what}: worst {float(uh.max()):.2f} tol units, fp32 oracle {float(uo.max()):.2f}; {int((uh > 1).sum())} of {n} rows "
           f"beyond (i), {int(only3.sum())} by (iii) only, {int(width.sum())} by the neighbourhood's width")
    bad = ~(ok12 | inside | only3)
    if bad.any():
        r = int(np.nonzero(bad)[0][np.argmax(eh[bad])])
        raise AssertionError(f"{msg}; {int(bad.sum())} rows pass no clause, worst row {r}: {uh[r]:.1f} units, fp32 oracle {uo[r]:.1f}")
    assert int(only3.sum()) <= n // 8, f"{msg}; more than {n // 8} rows need clause (iii)"
    if continuous and band is not None:                        # (`continuous`: a value that is continuous there - log q, y on `knots`)
        assert int(width.sum()) <= n // 8, f"{msg}; more than {n // 8} rows of a continuous value rely on the neighbourhood's width"
    return msg, float(uh.max()), float(uo.max()), int((uh > 1).sum()), int(only3.sum()), int(width.sum())


def plain_rule(what, a, o32, f64, spread=None):
    """(i), (ii) and - `spread` given - (iii), with the cap."""
    return band_rule(what, a, o32, f64, None, False, spread=spread)


def lazy_spread(of64, x64, g64):
    scale = max(1.0, float(g64.abs().max()))

    def f(rows):
        return sf.grad_spread(of64, x64[rows], g64[rows], scale, seed=int(rows[0]))
    return f


FAR = 100.0                                                   # rows with a coordinate beyond it (7.0 is not, 1e4 is) are judged apart:
                                                              # their log q of -5e7 would set the scale of every other row


def split_far(x):
    far = (x.abs() > FAR).any(1).numpy()
    return [s for s in (np.nonzero(~far)[0], np.nonzero(far)[0]) if len(s)]


@functools.lru_cache(maxsize=None)
def density_case(fam, D, H, circ, L, group, n=None):
    """Everything both test files need of one (case, group) of the density direction, computed once and never modified."""
    of, of64, _ = element_flow(fam, D, H, circ, L)
    rows = probe_rows(of64)[0]
    x = rows[group] if n is None else (rows[f"{group}{n}"] if n > len(rows[group]) else rows[group][:n])
    assert n is None or len(x) == n
    return _density(of, of64, x, band=group in ("knots", "edges"))


def _density(of, of64, x, band):
    lq64, g64 = logq_grad(of64, x.double())
    lq32, g32 = logq_grad(of, x)
    c = dict(of=of, of64=of64, x=x, lq64=lq64, g64=g64, lq32=lq32, g32=g32)
    if band:
        c["band_lq"], c["band_g"] = density_band(of64, x)
    return c


@functools.lru_cache(maxsize=None)
def sample_case(fam, D, H, circ, L, group, n=None):
    of, of64, _ = element_flow(fam, D, H, circ, L)
    draws = probe_rows(of64)[1]
    u, eps = draws[group] if n is None else (draws[f"{group}{n}"] if n > len(draws[group][0]) else tuple(t[:n] for t in draws[group]))
    assert n is None or len(u) == n
    return _sample(of, of64, u, eps, band=group in ("knots", "edges"))


def _sample(of, of64, u, eps, band):
    x64, ls64 = sample(of64, u.double(), eps.double())
    x32, ls32 = sample(of, u, eps)
    c = dict(of=of, of64=of64, u=u, eps=eps, x64=x64, ls64=ls64, x32=x32, ls32=ls32)
    if band:
        c["band_x"], c["band_ls"] = sample_band(of64, u, eps)
    return c


@functools.lru_cache(maxsize=None)
def deep_case(D, L, H, circ, level, n=DEEP_B):
    """The deep group: a flow whose conditioner matters, at its own float64 samples rounded to float32."""
    of, of64, seed = deep_flow(D, L, H, circ, level)
    g = torch.Generator().manual_seed(seed + 2)
    u, eps = torch.rand(n, D, generator=g), torch.randn(n, D, generator=g)
    c = _sample(of, of64, u, eps, band=False)
    c.update(_density(of, of64, c["x64"].float(), band=False))
    return c


def check_density(c, lq, g, group, fam=None, label="", gradient=True):
    """log q and d log q / dx of an implementation against case `c` under the rule of `group` (plain `close` on top where
    (fam, group, "lq") is in PLAIN); returns the report rows of band_rule."""
    from helpers import close, worst
    rep = []
    banded = group in ("knots", "edges")
    for rows in split_far(c["x"]) if group == "edges" else [np.arange(len(c["x"]))]:
        sel = lambda t: t[rows]                                 # noqa: E731
        spread = lazy_spread(c["of64"], c["x"].double()[rows], c["g64"][rows])
        bl, bg = [(lo[rows], hi[rows]) for lo, hi in (c["band_lq"], c["band_g"])] if banded else (None, None)
        if (fam, group, "lq") in PLAIN:
            assert close(sel(lq), sel(c["lq64"]), RTOL), f"{label}{group} log q: {worst(sel(lq), sel(c['lq64'])):.2f}x tol"
        rep.append(band_rule(f"{label}{group} log q", sel(lq), sel(c["lq32"]), sel(c["lq64"]), bl, continuous=group == "knots"))
        if gradient:
            rep.append(band_rule(f"{label}{group} d log q / dx", sel(g), sel(c["g32"]), sel(c["g64"]), bg, continuous=False,
                                 spread=spread))
    return rep


def check_sample(c, x, ls, group, fam=None, label=""):
    from helpers import close, worst
    rep = []
    banded = group in ("knots", "edges")
    for rows in split_far(c["eps"]) if group == "edges" else [np.arange(len(c["eps"]))]:
        sel = lambda t: t[rows]                                 # noqa: E731
        for q, name, a, o32, f64, bk in (("x", "x", x, c["x32"], c["x64"], "band_x"), ("ls", "log q", ls, c["ls32"], c["ls64"], "band_ls")):
            what = f"{label}sample {group} {name}"
            if (fam, group, q) in PLAIN:
                assert close(sel(a), sel(f64), RTOL), f"{what}: {worst(sel(a), sel(f64)):.2f}x tol"
            band = tuple(t[rows] for t in c[bk]) if banded else None
            rep.append(band_rule(what, sel(a), sel(o32), sel(f64), band, continuous=group == "knots"))
    return rep
