"""The spline case list (tests/spline_cases.py), asserted from the CPU oracle alone: what test_gpu_spline_cases.py takes for granted.
No GPU.

  * branch coverage: the float64 parameters reach the branches each family is named for, every bin holds an `interior` row, the
    `knots` rows fall on both sides of their knot under the float32 oracle;
  * oracle precision: the fp32 oracle against its float64 copy on every case, group and direction - inside a quarter of the
    tolerance wherever spline_cases.PLAIN says so (the GPU file asserts plain `close` there), and on E1 / E2 every row of log q
    inside clause (i) or the neighbourhood.  The figures of the other groups are printed: rows of E3 and of
    the E2 height knots (an inverse through a knot derivative of 1e-3) pass none of these for the ORACLE - an implementation meets
    them through clause (ii);
  * the stand-in for the kernels: the oracle with permuted hidden units (the same function in another summation order) passes every
    rule against float64 with the unpermuted oracle as `o32`, caps in force - on the deep group this is the admission test of a
    (shape, level);
  * mutants of a float32 restatement of the spline: each is >= 100 tolerances away on >= 25 % of the rows of some case and group."""
import contextlib
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spline_cases as sc
import stressed_flow as sf
from helpers import RTOL
from oracle import spline as osp

K = sc.K


@pytest.fixture(autouse=True)
def one_thread():
    """The fp32 oracle's sums follow the thread count; the GPU tests run it on one thread (tests/conftest.py), so this file does."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ---- branch coverage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,D,H,circ,L", sc.ELEMENT_CASES)
def test_the_parameters_reach_the_branches_of_their_family(fam, D, H, circ, L):
    of, of64, _ = sc.element_flow(fam, D, H, circ, L)
    for k, p in of.named_parameters():                         # the float64 copy holds the same float32-representable numbers
        assert torch.equal(dict(of64.named_parameters())[k].float(), p)
    for f in sc.couplings(of):
        assert not bool(f.prqct.transform_net.final_layer.weight.any())
    cov = sc.coverage(fam, of64)
    assert all(cov.values()), {k: v for k, v in cov.items() if not v}
    tb, circ_mask = sc.flow_meta(of64)
    assert torch.equal(tb.float(), sc.tail_bounds(D, circ)) and circ_mask.nonzero().flatten().tolist() == list(circ)
    if fam == "E2":                                            # the thresholds of sp_softplus sit between float32 neighbours of the list
        assert np.float32(20.001) > 20 > np.float32(19.999) and np.float32(-4.999) > -5 > np.float32(-5.001)


@pytest.mark.parametrize("fam,D,H,circ,L", sc.ELEMENT_CASES)
def test_the_probe_rows_sit_where_they_should(fam, D, H, circ, L):
    of, of64, _ = sc.element_flow(fam, D, H, circ, L)
    tb, cm = sc.flow_meta(of64)
    dens, samp = sc.probe_rows(of64)
    for direction, f, which in (("density", sc.first_density_layer, "w"), ("sample", sc.first_sample_layer, "h")):
        kn64 = sc.layer_knots(f(of64), tb, which)
        kn32 = sc.layer_knots(f(of), tb.float(), which)
        if direction == "density":
            rows = {g: dens[g] for g in sc.GROUPS}
        else:
            rows = {g: torch.where(cm, (samp[g][0] - 0.5) * of.q0.scale, samp[g][1]) for g in sc.GROUPS}
        # every one of the K bins, on every coordinate, holds interior rows - in float64 and under the float32 knots alike
        for kn, x in ((kn64, rows["interior"].double()), (kn32, rows["interior"])):
            b = sc.bins_of(kn, sc.wrap(x, tb.to(x.dtype), cm) if direction == "density" else x)
            assert torch.equal(b, torch.arange(K).repeat_interleave(3)[:, None].expand(-1, D)), direction
        for g, want in (("bin0", 0), ("binK", K - 1)):
            assert bool((sc.bins_of(kn32, rows[g]) == want).all()) and bool((sc.bins_of(kn64, rows[g].double()) == want).all())
        # knots rows: the three rows of inner knot j (the rounded knot, one ulp up, one down) fall into bins j - 1 and j under the
        # float32 oracle's own knots, on every coordinate that is not wrapped first
        xk = rows["knots"]
        b = sc.bins_of(kn32, xk).view(3, K - 1, D)
        j = torch.arange(1, K)[None, :, None]
        lin = ~cm if direction == "density" else torch.ones(D, dtype=torch.bool)
        assert bool(((b == j) | (b == j - 1))[:, :, lin].all())
        assert bool((b[1] == j[0])[:, lin].any()) and bool((b[2] == j[0] - 1)[:, lin].any())
        both = ((b == j).any(0) & (b == j - 1).any(0))[:, lin]
        # (the float32 knot is a rounded cumulative sum of up to K terms times 2 tb: it sits within a few ulps of the float64 knot, the
        # three rows span two - a knot has rows on both sides with a chance of about 2 in 2 x (a few): a quarter of the knots is the floor)
        assert float(both.float().mean()) >= 0.25, f"{direction}: only {float(both.float().mean()):.2f} of the knots have rows on both sides"
    assert len(dens["interior"]) == 3 * K and len(dens["knots"]) == 3 * (K - 1)
    e = dens["edges"]
    t = tb.float()
    assert torch.equal(e[0], t) and torch.equal(e[1], -t) and bool((e[2] < t).all()) and bool((e[3] > t).all())
    assert float(e[6, 0]) == 7.0 and float(e[7, 0]) == 1e4 and bool((e[8] == 0).all()) and bool(torch.signbit(e[9]).all())
    assert len(e) == (14 if circ else 10)
    # the sampling draws stay inside what the base distribution can produce
    for g in sc.GROUPS:
        u, eps = samp[g]
        assert bool(((u >= 0) & (u <= 1)).all()) and bool(torch.isfinite(eps).all())


# ---- oracle precision ------------------------------------------------------------------------------------------------------------------
def _oracle_report(a, f64, band=None, spread=None):
    """(worst units, rows beyond (i), rows inside the neighbourhood only, rows inside 4x the spread only, rows inside none, non-finite
    rows) of the fp32 oracle ALONE - clause (ii) does not exist for it."""
    e, u = sc.row_errs(a, f64)
    ok = u <= 1.0
    nb = np.zeros_like(ok)
    if band is not None:
        nb = sc.band_units(a, band[0], band[1], max(1.0, float(f64.abs().max()))) <= 1.0
    s3 = np.zeros_like(ok)
    if spread is not None and not (ok | nb).all():
        rows = np.nonzero(~(ok | nb))[0]
        s3[rows] = e[rows] <= 4 * np.asarray(spread(rows))
    fin = u[np.isfinite(u)]
    return dict(worst=float(fin.max()) if len(fin) else 0.0, beyond=int((~ok).sum()), nb=int((~ok & nb).sum()), iii=int(s3.sum()),
                none=int((~(ok | nb | s3)).sum()), nonfinite=int((~np.isfinite(u)).sum()), n=len(u))


@pytest.mark.parametrize("fam,D,H,circ,L", sc.ELEMENT_CASES)
def test_fp32_oracle_on_every_group_of_an_element_case(fam, D, H, circ, L):
    for grp in sc.GROUPS:
        banded = grp in ("knots", "edges")
        c = sc.density_case(fam, D, H, circ, L, grp)
        s = sc.sample_case(fam, D, H, circ, L, grp)
        for k in ("lq64", "g64"):
            assert bool(torch.isfinite(c[k]).all()), (grp, k)
        for k in ("x64", "ls64"):
            assert bool(torch.isfinite(s[k]).all()), (grp, k)
        for rows in (sc.split_far(c["x"]) if grp == "edges" else [np.arange(len(c["x"]))]):
            far = bool((c["x"][rows].abs() > sc.FAR).any())
            rep = {"lq": _oracle_report(c["lq32"][rows], c["lq64"][rows], tuple(t[rows] for t in c["band_lq"]) if banded else None),
                   "g": _oracle_report(c["g32"][rows], c["g64"][rows], tuple(t[rows] for t in c["band_g"]) if banded else None,
                                       sc.lazy_spread(c["of64"], c["x"].double()[rows], c["g64"][rows]))}
            print(f"{fam} D={D} L={L} density {grp}{' (far)' if far else ''}: " + "; ".join(
                f"{q} worst {r['worst']:.2f}, {r['beyond']} beyond (i), {r['nb']} nb, {r['iii']} (iii), {r['none']} none of {r['n']}"
                for q, r in rep.items()))
            if (fam, grp, "lq") in sc.PLAIN:
                assert rep["lq"]["worst"] <= 0.25, (grp, rep["lq"])
            assert rep["lq"]["nonfinite"] + rep["g"]["nonfinite"] == 0, (grp, rep)
            if fam in ("E1", "E2"):                            # log q of the oracle itself: every row inside (i) or the neighbourhood
                assert rep["lq"]["none"] == 0, (grp, rep)
        for rows in (sc.split_far(s["eps"]) if grp == "edges" else [np.arange(len(s["eps"]))]):
            rep = {"x": _oracle_report(s["x32"][rows], s["x64"][rows], tuple(t[rows] for t in s["band_x"]) if banded else None),
                   "ls": _oracle_report(s["ls32"][rows], s["ls64"][rows], tuple(t[rows] for t in s["band_ls"]) if banded else None)}
            print(f"{fam} D={D} L={L} sample {grp}: " + "; ".join(
                f"{q} worst {r['worst']:.2f}, {r['beyond']} beyond (i), {r['nb']} nb, {r['none']} none, {r['nonfinite']} non-finite of "
                f"{r['n']}" for q, r in rep.items()))
            for q in ("x", "ls"):
                if (fam, grp, q) in sc.PLAIN:
                    assert rep[q]["worst"] <= 0.25 and rep[q]["nonfinite"] == 0, (grp, q, rep[q])
            if not (fam == "E2" and grp == "knots"):
                # a NaN of the fp32 oracle where float64 is finite: only y on a height knot whose derivative is 1e-3 (the
                # discriminant b^2 - 4ac of the inverse rounds below zero)
                assert rep["x"]["nonfinite"] + rep["ls"]["nonfinite"] == 0, (grp, rep)


def test_the_plain_set_names_no_other_family():
    assert all(f in ("E1", "E2") for f, _, _ in sc.PLAIN)
    assert all(g in ("interior", "bin0", "binK") for _, g, _ in sc.PLAIN)
    assert {("E1", "interior", "x"), ("E2", "interior", "lq"), ("E2", "interior", "x")} <= sc.PLAIN


# ---- the stand-in for the kernels --------------------------------------------------------------------------------------------------------
def _twin_checks(c, tw, group, fam=None, density=True):
    rep = []
    if density:
        lq, g = sc.logq_grad(tw, c["x"])
        rep += sc.check_density(c, lq, g, group, fam)
    if "u" in c:
        x, ls = sc.sample(tw, c["u"], c["eps"])
        rep += sc.check_sample(c, x, ls, group, fam)
    return rep


@pytest.mark.parametrize("fam,D,H,circ,L", sc.ELEMENT_CASES)
def test_permuted_twin_passes_every_rule_on_an_element_case(fam, D, H, circ, L):
    """(With the final weight zero the conditioner's output is its bias in any summation order: on the element families the twin
    checks the rules' plumbing - caps, PLAIN, the far rows -, on the deep group below it is a second float32 evaluation.)"""
    of, of64, seed = sc.element_flow(fam, D, H, circ, L)
    tw = sc.permuted_twin(of, seed)
    for grp in sc.GROUPS:
        _twin_checks(sc.density_case(fam, D, H, circ, L, grp), tw, grp, fam)
        if not sc.hip_dropped("sample", fam, D, L, grp):       # (the comparisons the GPU file makes: on E2 `knots` draws the oracle - and
            _twin_checks(sc.sample_case(fam, D, H, circ, L, grp), tw, grp, fam, density=False)    # its twin - has a NaN row, which passes no clause)
    for grp, n in sc.RAGGED.items():
        assert len(sc.density_case(fam, D, H, circ, L, grp, n)["x"]) == n and len(sc.sample_case(fam, D, H, circ, L, grp, n)["u"]) == n


def _deep_cases():
    return [(D, L, H, circ, lv, n) for (D, L, H, circ) in sc.DEEP_SHAPES for lv in sc.DEEP_LEVELS
            for n in ((sc.DEEP_B, sc.DEEP_RAGGED) if (D, lv) == (12, sc.DEEP_LEVELS[0]) else (sc.DEEP_B,))]


@pytest.mark.parametrize("D,L,H,circ,level,n", _deep_cases())
def test_a_deep_level_is_kept_only_if_the_permuted_twin_passes(D, L, H, circ, level, n):
    c = sc.deep_case(D, L, H, circ, level, n)
    fin = all(bool(torch.isfinite(c[k]).all()) for k in ("lq64", "g64", "x64", "ls64"))
    gmax = float(c["g64"].abs().max())
    rep, ok, why = [], True, ""
    for seed in range(3):                                      # three summation orders: a level one of them leaves is marginal
        tw = sc.permuted_twin(c["of"], seed)
        with torch.no_grad():                                  # the twin IS another summation order: not bit-identical
            assert not torch.equal(tw.log_prob(c["x"]), c["lq32"])
        try:
            rep += _twin_checks(c, tw, "deep")
        except AssertionError as e:
            ok, why = False, why + f" [twin {seed}: {e}]"
    for r in rep:
        print(r[0])
    _, uo = sc.row_errs(c["lq32"], c["lq64"])
    _, ug = sc.row_errs(c["g32"], c["g64"])
    _, ux = sc.row_errs(c["x32"], c["x64"])
    print(f"deep D={D} L={L} H={H} level={level} n={n}: float64 finite {fin}, max|grad| {gmax:.2e}; fp32 oracle log q {uo.max():.2f}, "
          f"grad {ug.max():.1f} ({int((ug > 1).sum())} rows beyond (i)), sample x {ux.max():.2f}; twin passes: {ok} {why}")
    keep = fin and gmax < sc.DEEP_MAX_GRAD and ok
    assert keep == ((D, L, H, circ, level) not in sc.DEEP_DROPPED), (fin, gmax, ok, why)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("softplus saturates at 20", "MIN_DERIVATIVE dropped", "minimum bin width without (1 - K MIN)", "MIN_BIN_WIDTH = 0",
           "inverse searches the width knots", "forward searches the height knots", "circular end derivative not tied",
           "linear end derivatives left free")


RECIPROCALS = "quotients by reciprocal"       # not a mutant: the same function in another rounding


def _rqs(inputs, uw, uh, ud, inverse, left, right, bottom, top, mut):
    """oracle.spline.rational_quadratic_spline restated (mut = None: bit-identical, asserted below) with one-line mutants."""
    min_w = 0.0 if mut == "MIN_BIN_WIDTH = 0" else osp.MIN_BIN_WIDTH
    widths = F.softmax(uw, dim=-1)
    widths = min_w + (1.0 if mut == "minimum bin width without (1 - K MIN)" else (1 - min_w * K)) * widths
    cumwidths = F.pad(torch.cumsum(widths, dim=-1), pad=(1, 0), value=0.0)
    cumwidths = (right - left)[..., None] * cumwidths + left[..., None]
    cumwidths[..., 0] = left
    cumwidths[..., -1] = right
    widths = cumwidths[..., 1:] - cumwidths[..., :-1]
    sp = F.softplus(ud)
    if mut == "softplus saturates at 20":
        sp = torch.where(ud > 20, torch.full_like(ud, 20.0), sp)
    derivatives = (0.0 if mut == "MIN_DERIVATIVE dropped" else osp.MIN_DERIVATIVE) + sp
    heights = F.softmax(uh, dim=-1)
    heights = osp.MIN_BIN_HEIGHT + (1 - osp.MIN_BIN_HEIGHT * K) * heights
    cumheights = F.pad(torch.cumsum(heights, dim=-1), pad=(1, 0), value=0.0)
    cumheights = (top - bottom)[..., None] * cumheights + bottom[..., None]
    cumheights[..., 0] = bottom
    cumheights[..., -1] = top
    heights = cumheights[..., 1:] - cumheights[..., :-1]
    search_h = inverse
    if (mut == "inverse searches the width knots" and inverse) or (mut == "forward searches the height knots" and not inverse):
        search_h = not inverse
    bin_idx = osp._searchsorted(cumheights if search_h else cumwidths, inputs)[..., None].clamp(0, K - 1)
    g = lambda t: t.gather(-1, bin_idx)[..., 0]          # noqa: E731
    in_cw, in_w, in_ch, in_h = g(cumwidths), g(widths), g(cumheights), g(heights)
    rc = mut == RECIPROCALS                                  # quotients as products with a rounded reciprocal, as the kernels do
    delta = heights * (1 / widths) if rc else heights / widths
    in_delta, in_d, in_d1 = g(delta), g(derivatives), g(derivatives[..., 1:])
    if inverse:
        a = (inputs - in_ch) * (in_d + in_d1 - 2 * in_delta) + in_h * (in_delta - in_d)
        b = in_h * in_d - (inputs - in_ch) * (in_d + in_d1 - 2 * in_delta)
        c = -in_delta * (inputs - in_ch)
        disc = b.pow(2) - 4 * a * c
        root = (2 * c) * (1 / (-b - torch.sqrt(disc))) if rc else (2 * c) / (-b - torch.sqrt(disc))
        outputs = root * in_w + in_cw
        t1mt = root * (1 - root)
        denom = in_delta + (in_d + in_d1 - 2 * in_delta) * t1mt
        dnum = in_delta.pow(2) * (in_d1 * root.pow(2) + 2 * in_delta * t1mt + in_d * (1 - root).pow(2))
        return outputs, -(torch.log(dnum) - 2 * torch.log(denom))
    theta = (inputs - in_cw) * (1 / in_w) if rc else (inputs - in_cw) / in_w
    t1mt = theta * (1 - theta)
    numer = in_h * (in_delta * theta.pow(2) + in_d * t1mt)
    denom = in_delta + (in_d + in_d1 - 2 * in_delta) * t1mt
    outputs = in_ch + numer * (1 / denom) if rc else in_ch + numer / denom
    dnum = in_delta.pow(2) * (in_d1 * theta.pow(2) + 2 * in_delta * t1mt + in_d * (1 - theta).pow(2))
    return outputs, torch.log(dnum) - 2 * torch.log(denom)


def _unconstrained(mut):
    def f(inputs, uw, uh, ud, inverse, circ, tail_bound):
        const = math.log(math.exp(1 - osp.MIN_DERIVATIVE) - 1)
        ud = ud.clone()
        lin = ~circ
        if mut != "linear end derivatives left free":
            ud[..., lin, 0] = const
            ud[..., lin, -1] = const
        if mut != "circular end derivative not tied":
            ud[..., circ, -1] = ud[..., circ, 0]
        tb = torch.broadcast_to(tail_bound, inputs.shape)
        inside = (inputs >= -tb) & (inputs <= tb)
        outputs = inputs.clone()
        logabsdet = torch.zeros_like(inputs)
        if inside.any():
            o, l = _rqs(inputs[inside], uw[inside], uh[inside], ud[inside], inverse, -tb[inside], tb[inside], -tb[inside],
                        tb[inside], mut)
            outputs = outputs.masked_scatter(inside, o)
            logabsdet = logabsdet.masked_scatter(inside, l)
        return outputs, logabsdet
    return f


@contextlib.contextmanager
def mutant(mut):
    """The oracle's modules evaluate the restated spline (with mutant `mut`) instead of oracle.spline.unconstrained_rqs."""
    keep = osp.unconstrained_rqs
    osp.unconstrained_rqs = _unconstrained(mut)
    try:
        yield
    finally:
        osp.unconstrained_rqs = keep


def _mutant_distance(of, dens_x, u, eps, ref):
    """[(what, per-row units of the mutant's float32 result from the float64 reference)]"""
    with torch.no_grad():
        lq = of.log_prob(dens_x)
        x, ls = of.sample_eps(u, eps)
    return [("log q", sc.row_errs(lq, ref["lq64"])[1]), ("sample x", sc.row_errs(x, ref["x64"])[1]),
            ("sample log q", sc.row_errs(ls, ref["ls64"])[1])]


def _old_inputs(D, H, circ, L=1, B=64):
    """The oracle half of test_gpu_spline.make_pair(std = 0.4) at the same shape, with that file's inputs."""
    seed = D + L
    tb = torch.full((D,), 5.0)
    g = torch.Generator().manual_seed(seed)
    tb[list(circ)] = math.pi / (0.5 + torch.rand(len(circ), generator=g))
    torch.manual_seed(seed)
    of = osp.make_circular_coupled_flow(D, L, H, circ, tb, seed=seed)
    osp.randomize(of, 0.4, seed + 1)
    of64 = copy.deepcopy(of).double()
    g = torch.Generator().manual_seed(5)
    u, eps = torch.rand(B, D, generator=g), torch.randn(B, D, generator=g)
    with torch.no_grad():
        x64, ls64 = of64.sample_eps(u.double(), eps.double())
        xq = x64.float() + 0.3 * torch.randn(B, D, generator=g)
        lq64 = of64.log_prob(xq.double())
    return of, xq, u, eps, dict(lq64=lq64, x64=x64, ls64=ls64)


def test_the_restated_spline_is_the_oracle_bit_for_bit():
    for case in sc.ELEMENT_CASES[:12:3]:
        of = sc.element_flow(*case)[0]
        c, s = sc.density_case(*case, "knots"), sc.sample_case(*case, "interior")
        with mutant(None), torch.no_grad():
            assert torch.equal(of.log_prob(c["x"]), c["lq32"])
            x, ls = of.sample_eps(s["u"], s["eps"])
        assert torch.equal(x, s["x32"]) and torch.equal(ls, s["ls32"])


@pytest.mark.parametrize("mut", MUTANTS)
def test_a_mutant_is_far_away_on_some_case_and_group(mut):
    best = (0.0, None)
    for case in [c for c in sc.ELEMENT_CASES if c[4] == 1]:
        of = sc.element_flow(*case)[0]
        for grp in sc.GROUPS:
            c, s = sc.density_case(*case, grp), sc.sample_case(*case, grp)
            near_d = sc.split_far(c["x"])[0] if grp == "edges" else slice(None)
            near_s = sc.split_far(s["eps"])[0] if grp == "edges" else slice(None)
            ref = dict(lq64=c["lq64"][near_d], x64=s["x64"][near_s], ls64=s["ls64"][near_s])
            with mutant(mut):
                for what, u in _mutant_distance(of, c["x"][near_d], s["u"][near_s], s["eps"][near_s], ref):
                    frac = float((u >= 100).mean())
                    if frac > best[0]:
                        best = (frac, f"{case} {grp} {what}: {int((u >= 100).sum())} of {len(u)} rows, worst {float(u.max()):.0f} units")
    old = []
    for (D, H, circ) in sc.E_SHAPES:
        of, xq, u, eps, ref = _old_inputs(D, H, circ)
        with mutant(mut):
            for what, un in _mutant_distance(of, xq, u, eps, ref):
                old.append((float((un >= 100).mean()), float(un.max()), f"D={D} {what}"))
    o = max(old)
    print(f"mutant '{mut}': new cases {best[1]}; on make_pair(std = 0.4) inputs at most {100 * o[0]:.0f} % of the rows beyond 100 units "
          f"({o[2]}), worst row {max(v[1] for v in old):.1f} units")
    assert best[0] >= 0.25, f"'{mut}': at most {100 * best[0]:.0f} % of the rows of any case and group are 100 tolerances away ({best[1]})"


@pytest.mark.parametrize("fam,D,H,circ,L", sc.ELEMENT_CASES)
def test_reciprocal_twin_passes_every_comparison_the_gpu_file_makes(fam, D, H, circ, L):
    """A float32 evaluation of the element families that DOES differ from the oracle (the permuted twin does not, with the final
    weight zero): every quotient of the restated spline as a product with a rounded reciprocal, the kernels' form.  It passes every
    rule, caps in force, on every comparison of density and sampling that test_gpu_spline_cases.py makes; what it gives on the
    sampling comparisons of spline_cases.HIP_DROPPED is printed (it leaves the rule on E2 `knots` draws, and stays inside it on E3,
    where one changed rounding per quotient is not the kernels' 1 - 2 ulp exp / log / rcp forms)."""
    of = sc.element_flow(fam, D, H, circ, L)[0]
    for grp in sc.GROUPS:
        with mutant(RECIPROCALS):
            _twin_checks(sc.density_case(fam, D, H, circ, L, grp), of, grp, fam)
            try:
                _twin_checks(sc.sample_case(fam, D, H, circ, L, grp), of, grp, fam, density=False)
            except AssertionError as e:
                if not sc.hip_dropped("sample", fam, D, L, grp):
                    raise
                print(f"reciprocal twin on a dropped comparison, {fam} D={D} L={L} sample {grp}: {str(e)[:300]}")
    with mutant(RECIPROCALS), torch.no_grad():                 # another rounding, not the same bits
        s = sc.sample_case(fam, D, H, circ, L, "interior")
        assert not torch.equal(of.sample_eps(s["u"], s["eps"])[0], s["x32"])


# ---- special rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,D,H,circ,L", sc.ELEMENT_CASES)
def test_special_rows_in_float64_and_float32(fam, D, H, circ, L):
    """A NaN or infinite coordinate: outside every spline (the identity branch).  A linear coordinate reaches the Gaussian base: NaN
    gives NaN, +-inf gives -inf - or NaN where the coordinate conditions another one (0 * inf in the conditioner's final layer).  A
    circular coordinate is wrapped first (remainder: NaN for all three) and the uniform base ignores its value: NaN where the
    coordinate conditions another one, else finite.  float32 and float64 agree on the pattern, and the rows without a special value
    are finite."""
    of, of64, _ = sc.element_flow(fam, D, H, circ, L)
    dens, _ = sc.probe_rows(of64)
    x, sp = dens["special"], dens["special_rows"]
    with torch.no_grad():
        l64, l32 = of64.log_prob(x.double()), of.log_prob(x)
    rest = [i for i in range(len(x)) if i not in sp]
    assert bool(torch.isfinite(l64[rest]).all()) and bool(torch.isfinite(l32[rest]).all())
    assert torch.equal(torch.isnan(l64), torch.isnan(l32)) and torch.equal(l64 == -math.inf, l32 == -math.inf)
    assert not bool((l64 == math.inf).any())
    assert bool(torch.isnan(l64[sp[0]]))                                                       # the linear coordinate
    assert bool((l64[sp[1]] == -math.inf) | torch.isnan(l64[sp[1]])) and bool(torch.equal(torch.isnan(l64[sp[1]]), torch.isnan(l64[sp[2]])))
    pat = ["nan" if math.isnan(v) else ("-inf" if v == -math.inf else "finite") for v in l64[sp].tolist()]
    print(f"special rows D={D} L={L} circ={circ}: {pat}")
    if circ:
        assert all(p in ("nan", "finite") for p in pat[3:]) and len(set(pat[3:])) == 1
