"""Cases for the native GMM and ManyWell targets away from the reference's one configuration (test_target_cases.py asserts
every claim made here from the restatements alone; test_gpu_targets.py runs every HIP route on them) - TEST INFRASTRUCTURE, CPU only.

The reference's GMM has ONE scale, softplus(log_var_scaling), for every component k and coordinate j, at D = 2 and n_mix = 40:
with equal scales a read of scales[k][0] for every j, of scales[0][j] for every k, a transposed read, a dropped half log
determinant (a constant then) and log(sc) summed over the wrong index all give the bits of the correct code.  Its ManyWell is
only ever a, b, c = -0.5, -6, 1 without a normalisation constant.  The C ABI (fabhip_target) takes locs[n_mix][D] and
scales[n_mix][D] per entry, and a, b, c, log_norm.

csrc/target_device.h: target_tile is the ONE device function of both targets.  Its call sites and the route that reaches each:
  reduce_kernels.hip   k_target<true> / <false>            target.log_prob_and_grad / target.log_prob (fabhip_target_log_prob); the
                                                           generic path's plug-in evaluation; the step-by-step spline path
  ais_tile16.hip       ais_init_body (k_ais_init*)         chain initialisation of the fused call, 16-chain tiles, MIX too
                       hmc_step_body (k_hmc_step*, _mix)   16-chain HMC tiles (FABHIP_OPT_TILE_SHAPE 16), the defensive mixture
  ais_tile48.hip       k_hmc_step_r4 / k_ais_init_r4       4-chain tiles: fused stages / staged / stream (FABHIP_OPT_R4_STREAM 2 / 0 / 1)
                       k_hmc_step_r8 / k_ais_init_r8       8-chain tiles
  ais_tile16_metropolis.hip  create_point_body             fabhip_create_point
                       metropolis_body                     target_tile<false> on every proposal (fabhip_metropolis_transition)
  spline_r8.h          the host-fused spline transition    target_tile<true> on the moved point of every leapfrog

RESTATEMENT.  `GMMStatement` / `ManyWellStatement` write log p AND its gradient out (float64 or float32), with every place a
wrong index or factor could sit as a one-line method, so that a mutant is a one-line override.  test_target_cases.py pins them
to oracle/targets.py (which fixture g3 pins to the reference): bit-near equal log p, gradient = float64 autograd.

GMM ROWS, per case three groups of B_ROWS = 48 float32-representable rows kept apart (the absolute floor of `helpers.close` is
2e-6 of the largest entry of the tensor compared: a far-field gradient of 300 next to a near-field one of 0.1 would hide it):
  near     x = loc_k + 0.6 scale_k * noise for k = i % n_mix: every lane slot k % 16 is the arg-max of some row
  between  on the segment from loc_a to its nearest neighbour loc_b, at the point where the two components differ by a drawn
           delta in [-2.5, 2.5]: the second responsibility is >= 0.05 on most rows (near field: |log p| stays below ~1e3)
  far      on a ray from a mean, at the distance where log p hits a level: 16 levels in [-4000, -max(30, 2.5 D)], 16 in [-9800, -5000]
           (live just short of the mask), 16 in [-30000, -10200] (masked); a draw is kept only if the second responsibility is
           below 1e-3 (with equal scales a far-field row on the tie line of two components is 9 - 24 tolerances off in float32
           whichever way the responsibilities are formed) and no row is within 1 % of -1e4.  The rows are shuffled, so that a
           slice of any length holds live and masked rows side by side.
  special  one NaN coordinate, one +inf coordinate, one row of zeros.

TRANSITION CASES.  The seeded flows of hmc_mass_cases.SHAPES with a GMM whose means are samples of that flow (inside its sample
spread), unit mass, max_grad = 1e3, n_outer = 2, beta 0.25 -> 0.5; (2, 2, 40) with 5 components; a Metropolis case at D = 5
with 17 components; whole calls of M = 3.  Step size, leapfrogs and seed per shape are chosen from the oracle alone so that the
conditions of test_target_cases.py hold.
"""
import copy
import functools
import math

import numpy as np
import torch

import hmc_mass_cases as mc
from helpers import seeded_oracle_flow
from oracle import ais as oais
from oracle import targets as otgt

MASK = -1e4
B_ROWS = 48
INF = float("inf")
DEFAULT_ABC = (-0.5, -6.0, 1.0)


class _WithGradient(torch.autograd.Function):
    """log p of a statement as an autograd node whose backward is the statement's OWN written-out gradient: the oracle's
    create_point differentiates log_p_fn, so a mutant of the gradient reaches the transition."""

    @staticmethod
    def forward(ctx, stmt, x):
        lp, g = stmt.log_prob_and_grad(x.detach())
        ctx.save_for_backward(g)
        return lp

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return None, grad_out[:, None] * g


class _Statement:
    def log_prob(self, x):
        if torch.is_grad_enabled() and x.requires_grad:
            return _WithGradient.apply(self, x)
        return self.log_prob_and_grad(x)[0]


class GMMStatement(_Statement):
    """Equal-weight mixture of diagonal normals N(locs[k], diag(scales[k])^2) with the reference's mask (gmm.py:57-66):
    comp_k = -(D log 2 pi + sum_j z_kj^2) / 2 - sum_j log s_kj - log n_mix, z_kj = (x_j - loc_kj) / s_kj;
    log p = logsumexp_k comp_k, + (-inf) where that is below -1e4;  d log p / dx_j = sum_k softmax(comp)_k (-(x_j - loc_kj) / s_kj^2),
    computed BEFORE the mask, as autograd through the reference's `lp + mask` gives it."""

    def __init__(self, locs, scales, dtype=torch.float64):
        assert locs.shape == scales.shape and locs.dim() == 2
        self.n_mix, self.dim = locs.shape
        self.locs, self.scales, self.dtype = locs.to(dtype), scales.to(dtype), dtype

    # ---- the one-line places -----------------------------------------------------------------------------------------------
    def _sc(self):
        return self.scales

    def _half_log_det(self, sc):
        return sc.log().sum(-1)

    def _log_mix(self):
        return -math.log(self.n_mix)

    def _components(self, comp):
        return comp

    def _grad_divisor(self, sc):
        return sc * sc

    def _grad_on_masked(self, g, masked):
        return g

    # -----------------------------------------------------------------------------------------------------------------------
    def parts(self, x):
        """(log p with the mask, gradient, responsibilities [B, n_mix], log p before the mask)"""
        x, sc = x.to(self.dtype), self._sc()
        diff = x[:, None, :] - self.locs[None]                                       # [B, n_mix, D]
        z = diff / sc[None]
        comp = self._components(-0.5 * (self.dim * math.log(2 * math.pi) + (z * z).sum(-1)) - self._half_log_det(sc)[None]
                                + self._log_mix())
        raw = torch.logsumexp(comp, -1)
        w = torch.softmax(comp, -1)
        g = (w[:, :, None] * (-diff / self._grad_divisor(sc)[None])).sum(1)
        mask = torch.zeros_like(raw)
        mask[raw < MASK] = -INF                                                      # gmm.py:63-65
        return raw + mask, self._grad_on_masked(g, raw < MASK), w, raw

    def log_prob_and_grad(self, x):
        return self.parts(x)[:2]


# ---- GMM mutants: the statement with ONE line changed -----------------------------------------------------------------------------
class ScaleOfFirstCoordinate(GMMStatement):
    def _sc(self):
        return self.scales[:, :1].expand(self.n_mix, self.dim)


class ScaleOfFirstComponent(GMMStatement):
    def _sc(self):
        return self.scales[:1].expand(self.n_mix, self.dim)


class ScalesReadTransposed(GMMStatement):
    def _sc(self):
        return self.scales.reshape(self.dim, self.n_mix).T


class HalfLogDetDropped(GMMStatement):
    def _half_log_det(self, sc):
        return torch.zeros(self.n_mix, dtype=self.dtype)


class ComponentsBeyondSixteenDropped(GMMStatement):
    def _components(self, comp):
        return comp.masked_fill(torch.arange(self.n_mix) >= 16, -INF)


class ScaleNotSquaredInGradient(GMMStatement):
    def _grad_divisor(self, sc):
        return sc


class LogMixDropped(GMMStatement):
    def _log_mix(self):
        return 0.0


class GradientZeroOnMaskedRows(GMMStatement):
    def _grad_on_masked(self, g, masked):
        return torch.where(masked[:, None], torch.zeros_like(g), g)


# name -> (class, where it shows: "both" / "log_p" / "grad", can differ at (D, n_mix), needs masked rows)
GMM_MUTANTS = {
    "scales[k][0] for every j": (ScaleOfFirstCoordinate, "both", lambda D, n: D > 1, False),
    "scales[0][j] for every k": (ScaleOfFirstComponent, "both", lambda D, n: n > 1, False),
    "scales read as [D][n_mix]": (ScalesReadTransposed, "both", lambda D, n: D > 1 and n > 1, False),
    "hld dropped": (HalfLogDetDropped, "both", lambda D, n: True, False),
    "components k >= 16 dropped": (ComponentsBeyondSixteenDropped, "both", lambda D, n: n > 16, False),
    "sc for sc * sc in the gradient": (ScaleNotSquaredInGradient, "grad", lambda D, n: True, False),
    "log_mix dropped": (LogMixDropped, "log_p", lambda D, n: n > 1, False),
    "gradient zeroed on masked rows": (GradientZeroOnMaskedRows, "grad", lambda D, n: True, True),
}


class ManyWellStatement(_Statement):
    """log p = -sum_i (a x_2i + b x_2i^2 + c x_2i^4 + x_(2i+1)^2 / 2) - log_norm (many_well.py:81-90, double_well.py:44-58)."""

    def __init__(self, dim, a=-0.5, b=-6.0, c=1.0, log_norm=0.0, dtype=torch.float64):
        assert dim % 2 == 0
        self.dim, self.a, self.b, self.c, self.log_norm, self.dtype = dim, a, b, c, log_norm, dtype

    def _abc(self):
        return self.a, self.b, self.c

    def _quartic_factor(self):
        return 4.0

    def _normalise(self, lp):
        return lp - self.log_norm

    def log_prob_and_grad(self, x):
        x = x.to(self.dtype)
        a, b, c = self._abc()
        xe, xo = x[:, 0::2], x[:, 1::2]
        x2 = xe * xe
        lp = -(a * xe + b * x2 + c * (x2 * x2)).sum(-1) - 0.5 * (xo * xo).sum(-1)
        g = torch.empty_like(x)
        g[:, 0::2] = -(a + 2.0 * b * xe + self._quartic_factor() * c * (x2 * xe))
        g[:, 1::2] = -xo
        return self._normalise(lp), g


class QuadraticAndQuarticSwapped(ManyWellStatement):
    def _abc(self):
        return self.a, self.c, self.b


class LogNormAdded(ManyWellStatement):
    def _normalise(self, lp):
        return lp + self.log_norm


class QuarticGradientWithoutFour(ManyWellStatement):
    def _quartic_factor(self):
        return 1.0


# "+ log_norm" moves log p by 2 log_norm: against |log p| of up to D / 2 wells that is 100 tolerances of `helpers.close` on a quarter
# of the rows around the wells up to this dimension only (asserted at every D up to it); beyond, the mutant shows in units of less
# than 100 tolerances, and the GPU file's comparison at `close` still sees it
LOG_NORM_SHOWS_UP_TO = 18
MANYWELL_MUTANTS = {"b and c swapped": (QuadraticAndQuarticSwapped, "both"), "+ log_norm": (LogNormAdded, "log_p"),
                    "quartic gradient without its factor 4": (QuarticGradientWithoutFour, "grad")}


# ---- GMM cases --------------------------------------------------------------------------------------------------------------------
# D: < 16 | = 16 | 17 .. 32 | 33 | 60 | 64 = FABHIP_MAX_DIM;  n_mix: 1, 3, 5, 7 (lanes without a component), 16, 17, 33, 40, 50, 64
GMM_SHAPES = [(1, 1), (2, 5), (2, 40), (5, 3), (6, 16), (7, 17), (16, 33), (32, 40), (33, 7), (60, 50), (64, 64)]
REFERENCE_CASE = (2, 40, 40.0, 1.0)                     # the reference's own (dim, n_mixes, loc_scaling, log_var_scaling)


def far_levels(D):
    """-log p of the far rows: from 30 (at least 2.5 D: the density AT a mean is already about -D) down past the mask"""
    return np.concatenate([np.geomspace(max(30.0, 2.5 * D), 4000.0, 16), np.linspace(5000.0, 9800.0, 16),
                           np.geomspace(10200.0, 30000.0, 16)])



def loc_scaling(D, n_mix):
    """half-width of the cube the means are drawn in: a few scales between neighbours at every (D, n_mix) - the distance of two
    uniform draws grows with sqrt(D), so the cube shrinks with it (the "between" rows are to stay in the near field)"""
    return float(min(40.0, min(4.0, max(1.0, 12.0 / math.sqrt(D))) * n_mix ** (1.0 / D)))


def draw_scales(n_mix, D, seed):
    """float32 [n_mix, D], log-uniform in [0.4, 1.6], all distinct"""
    g = torch.Generator().manual_seed(4000 + seed)
    while True:                                               # (a few thousand float32 draws do collide now and then: draw again)
        s = torch.exp(torch.empty(n_mix, D, dtype=torch.float64).uniform_(math.log(0.4), math.log(1.6), generator=g)).float()
        if len(set(s.reshape(-1).tolist())) == n_mix * D:
            return s


def _bisect(f, lo, hi, n=80):
    """per row: t in [lo, hi] with f(t) = 0 for f decreasing in t (float64 tensors)"""
    for _ in range(n):
        mid = 0.5 * (lo + hi)
        pos = f(mid) > 0
        lo, hi = torch.where(pos, mid, lo), torch.where(pos, hi, mid)
    return 0.5 * (lo + hi)


def component_of_row(K, B=B_ROWS):
    """the component row i is drawn around: i % K up to 16 components; beyond, every third row goes round the components
    k >= 16 (a third of the rows then sit in a component that lanes reach only in their second pass) and the others round 0 .. 15"""
    i = torch.arange(B)
    if K <= 16:
        return i % K
    return torch.where(i % 3 == 2, 16 + (i // 3) % (K - 16), (i - i // 3) % 16)


def _rows(st, g):
    """the three groups of B_ROWS rows and the special rows for the float64 statement `st` (generator g)"""
    K, D, B = st.n_mix, st.dim, B_ROWS
    locs, sc = st.locs, st.scales
    k = component_of_row(K)
    near = locs[k] + 0.6 * sc[k] * torch.randn(B, D, generator=g, dtype=torch.float64)
    # between: from loc_a towards its nearest neighbour b, where comp_a - comp_b = delta
    a = torch.arange(B) % K
    d2 = ((locs[:, None] - locs[None]) ** 2).sum(-1) + torch.eye(K, dtype=torch.float64) * 1e30
    b = d2.argmin(1)[a] if K > 1 else a
    delta = torch.empty(B, dtype=torch.float64).uniform_(-2.5, 2.5, generator=g)
    hld = sc.log().sum(-1)

    def gap(t):
        x = locs[a] + t[:, None] * (locs[b] - locs[a])
        ca = -0.5 * (((x - locs[a]) / sc[a]) ** 2).sum(-1) - hld[a]
        cb = -0.5 * (((x - locs[b]) / sc[b]) ** 2).sum(-1) - hld[b]
        return (ca - cb) - delta
    t = _bisect(gap, torch.zeros(B, dtype=torch.float64), torch.ones(B, dtype=torch.float64)) if K > 1 else torch.full((B,), 0.3, dtype=torch.float64)
    between = locs[a] + t[:, None] * (locs[b] - locs[a]) + 0.05 * torch.randn(B, D, generator=g, dtype=torch.float64)
    if K == 1:
        between = locs[a] + 2.0 * sc[a] * torch.randn(B, D, generator=g, dtype=torch.float64)
    # far: rays from a mean to the distance where log p = -level, kept if one component dominates
    far = torch.empty(B, D, dtype=torch.float64)
    for i, level in enumerate(far_levels(D)):
        centre = locs[k[i]]
        for attempt in range(200):
            u = torch.randn(1, D, generator=g, dtype=torch.float64)
            u = u / u.norm()
            r = _bisect(lambda r: st.parts(centre[None] + r[:, None] * u)[3] + level, torch.zeros(1, dtype=torch.float64),
                        torch.full((1,), 1e4, dtype=torch.float64))
            x = (centre[None] + r[:, None] * u).float().double()
            _, _, w, raw = st.parts(x)
            second = float(w.sort(-1).values[0, -2]) if K > 1 else 0.0
            if second < 1e-3 and abs(float(raw) + level) < 0.02 * level and abs(float(raw) - MASK) > 0.01 * abs(MASK):
                break
        else:
            raise AssertionError(f"no far row at level {level}")
        far[i] = x[0]
    far = far[torch.randperm(B, generator=g)]
    special = locs[torch.arange(3) % K] + 0.5 * torch.randn(3, D, generator=g, dtype=torch.float64)
    special[0, D // 2] = float("nan")
    special[1, D - 1] = INF
    special[2] = 0.0
    return {n: v.float().double() for n, v in (("near", near), ("between", between), ("far", far), ("special", special))}


GROUPS = ("near", "between", "far")


@functools.lru_cache(maxsize=None)
def gmm_case(D, n_mix, reference=False):
    """dict(locs, scales (float32), st64, st32, rows {group: float64 [B, D] at float32-representable values},
    ref {group: (log p, gradient, responsibilities, log p before the mask) in float64})."""
    g = torch.Generator().manual_seed(3000 + 64 * D + n_mix + (7 if reference else 0))
    if reference:
        o = otgt.GMM(*REFERENCE_CASE)
        locs, scales = o.locs.float(), o.scales.float()
    else:
        locs = ((torch.rand(n_mix, D, generator=g, dtype=torch.float64) - 0.5) * 2 * loc_scaling(D, n_mix)).float()
        scales = draw_scales(n_mix, D, 64 * D + n_mix)
    st64, st32 = GMMStatement(locs, scales), GMMStatement(locs, scales, torch.float32)
    rows = _rows(st64, g)
    ref = {n: st64.parts(x) for n, x in rows.items()}
    return dict(D=D, n_mix=n_mix, locs=locs, scales=scales, st64=st64, st32=st32, rows=rows, ref=ref)


def all_gmm_cases():
    return [(D, n, False) for D, n in GMM_SHAPES] + [(REFERENCE_CASE[0], REFERENCE_CASE[1], True)]


def grad_units(a, b):
    """per row: worst gradient element in tolerance units, NaN-proof (mc.tol_units on rows whose reference is finite)"""
    return mc.tol_units(torch.nan_to_num(a.double(), nan=0.0, posinf=0.0, neginf=0.0), b)


# ---- ManyWell cases ---------------------------------------------------------------------------------------------------------------
MW_DIMS = (2, 6, 18, 34, 64)
MW_ABC = (DEFAULT_ABC, (0.7, -3.0, 0.5))
MW_LOG_NORMS = ("zero", "log_Z", 3.25)          # 0 | the reference's log Z of the default wells (normalised=True) | an arbitrary one


def mw_log_norm(D, which):
    return 0.0 if which == "zero" else (otgt.ManyWell(D).log_Z if which == "log_Z" else float(which))


@functools.lru_cache(maxsize=None)
def manywell_rows(D):
    """{"wide": |x| up to 4, uniform; "modes": around the wells (+-1.7, 0); "special": NaN / +inf / -inf on a quartic and on a
    quadratic coordinate}, float64 at float32-representable values"""
    g = torch.Generator().manual_seed(5000 + D)
    wide = torch.empty(B_ROWS, D, dtype=torch.float64).uniform_(-4.0, 4.0, generator=g)
    wide[0, 0], wide[1, D - 2], wide[2, D - 1] = 4.0, -4.0, 4.0
    modes = torch.randn(B_ROWS, D, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(B_ROWS, D // 2, generator=g) < 0.3, -1.0, 1.0).double()
    modes[:, 0::2] = 1.7 * sign + 0.3 * modes[:, 0::2]
    special = torch.randn(6, D, generator=g, dtype=torch.float64)
    for r, (j, v) in enumerate(((0, float("nan")), (D - 1, float("nan")), (D - 2, INF), (1, INF), (0, -INF), (D - 1, -INF))):
        special[r, j] = v
    return {n: v.float().double() for n, v in (("wide", wide), ("modes", modes), ("special", special))}


def all_manywell_cases():
    return [(D, abc, ln) for D in MW_DIMS for abc in MW_ABC for ln in MW_LOG_NORMS]


def manywell_statement(D, abc, which, dtype=torch.float64, cls=ManyWellStatement):
    return cls(D, *abc, log_norm=mw_log_norm(D, which), dtype=dtype)


# ---- transition cases -------------------------------------------------------------------------------------------------------------
N_OUTER, ALPHA, BETA, BETA_NEXT = mc.N_OUTER, mc.ALPHA, mc.BETA, mc.BETA_NEXT
MW = "manywell"
# (D, K, nodes, B, n_mix): hmc_mass_cases.SHAPES and (2, 2, 40) with the 5 components of test_small_tiles_match_sixteen_chain_tiles
T_SHAPES = [(6, 3, 8, 37, 3), (32, 2, 16, 37, 33), (32, 10, 10, 37, 40), (60, 2, 4, 20, 50), (6, 2, 40, 37, 16), (2, 2, 40, 37, 5)]
T_TILES = {**mc.TILES, (2, 2, 40): (16, 4)}            # (W = 80 is below the 8-chain kernel's widths)
# per shape: (seed, step size, leapfrogs), chosen from the float64 oracle so that the conditions of test_target_cases.py hold
T_PARAMS = {(6, 3, 8): (1, 0.8, 5), (32, 2, 16): (0, 0.5, 3), (32, 10, 10): (21, 0.35, 3), (60, 2, 4): (1, 0.6, 5),
            (6, 2, 40): (3, 0.6, 3), (2, 2, 40): (2, 1.0, 3), (5, 2, 4): (0, 0.5, 2), (20, "plugin", 0): (2, 0.8, 5),
            (60, "spline", 0): (4, 0.03, 3), (MW, 6, 3, 8): (0, 0.5, 3),
            ("call", 32, 10, 10): (5, 0.4, 5), ("call", 60, 2, 4): (1, 0.6, 5)}     # (the step size of a call is CHAIN_EPS)
METROPOLIS_SHAPE = (5, 2, 4, 37, 17)            # (D, K, nodes, B, n_mix); step size = max_step_size, leapfrogs = n_updates
EXTRA_SHAPES = [(20, mc.PLUGIN, 0, 24, 9), (60, mc.SPLINE, 0, 20, 7)]       # the generic path's base / the spline flow
# in place of n_mix: ManyWell with the second (a, b, c) of the cases and a normalisation constant no property hands out
MW_T_SHAPE = (6, 3, 8, 37, MW)                  # tiles 16 and 4
MW_T_ARGS = MW_ABC[1] + (3.25,)


@functools.lru_cache(maxsize=None)
def t_inputs(D, K, nodes, B, n_mix, variant=None):
    """flow (float32 / float64), GMM statement pair with means = samples of the flow, float64 start point, noise.
    `variant`: another entry of T_PARAMS for the same shape (the whole calls have their own flow seed and leapfrog count)."""
    seed, eps, L = T_PARAMS[(variant, D, K, nodes) if variant else ((D, K, nodes) if n_mix != MW else (MW, D, K, nodes))]
    g = torch.Generator().manual_seed(7100 + seed + D + (K if isinstance(K, int) else len(K)))
    eps0 = torch.randn(B, D, generator=g)
    eps_l = torch.randn(n_mix if n_mix != MW else 1, D, generator=g)
    noise_p = torch.randn(N_OUTER, B, D, generator=g)
    noise_e = torch.empty(N_OUTER, B).exponential_(generator=g)
    extra = {}
    if K == mc.PLUGIN:
        nf = nf64 = mc.PlugGaussian(D)
        x, locs = (nf.scale * 0.5 * eps0.double()).float().double(), (nf.scale * 0.5 * eps_l.double()).float()
    elif K == mc.SPLINE:
        nf, nf64, tb = mc.spline_pair(D)
        u, u_l = torch.rand(B, D, generator=g), torch.rand(n_mix, D, generator=g)
        with torch.no_grad():
            x = nf64.sample_eps(u.double(), eps0.double())[0].float().double()
            locs = nf64.sample_eps(u_l.double(), eps_l.double())[0].float()
        extra = dict(tail_bound=tb)
    else:
        nf = seeded_oracle_flow(D, K, nodes, 600 + seed + D + K)
        nf64 = copy.deepcopy(nf).double()
        with torch.no_grad():
            x = nf64.sample_eps(eps0.double())[0].float().double()                 # float32-representable
            locs = nf64.sample_eps(eps_l.double())[0].float()                       # inside the flow's sample spread
    if n_mix == MW:
        locs = scales = None
        make = lambda dtype, cls=ManyWellStatement: cls(D, *MW_T_ARGS, dtype=dtype)                     # noqa: E731
    else:
        scales = draw_scales(n_mix, D, 900 + seed + D + n_mix)
        make = lambda dtype, cls=GMMStatement: cls(locs, scales, dtype)                                  # noqa: E731
    st64, st32 = make(torch.float64), make(torch.float32)
    start = oais.create_point(x, nf64.log_prob, st64.log_prob, True)
    proto = oais.HMC(1, D, None, None, alpha=ALPHA, epsilon=eps, n_outer=N_OUTER, L=L)     # the step sizes as float32 holds them
    return dict(nf=nf, nf64=nf64, locs=locs, scales=scales, st64=st64, st32=st32, start=start, noise_p=noise_p, noise_e=noise_e,
                eps=proto.epsilons.clone(), ceps=proto.common_epsilon.clone(), L=L, epsilon=eps, eps0=eps0, n_mix=n_mix,
                mass=torch.ones(D), max_grad=1e3, make=make, **extra)


def run_oracle(D, K, nodes, B, n_mix, dtype=torch.float64, target_cls=None):
    """One transition (N_OUTER outer steps) of the oracle HMC from the case's start point with `target_cls` as its target."""
    c = t_inputs(D, K, nodes, B, n_mix)
    nf = c["nf64"] if dtype == torch.float64 else c["nf"]
    tgt = c["make"](dtype) if target_cls is None else c["make"](dtype, target_cls)
    h = mc.CountingHMC(1, D, nf.log_prob, tgt.log_prob, alpha=ALPHA, p_target=False, epsilon=c["epsilon"], n_outer=N_OUTER,
                       L=c["L"], eval_mode=True, dtype=dtype)
    h.epsilons, h.common_epsilon = c["eps"].to(dtype).clone(), c["ceps"].to(dtype).clone()
    start = c["start"]
    if target_cls is not None:                                # a mutant starts from ITS point, as a kernel with that error would
        start = oais.create_point(c["start"].x, c["nf64"].log_prob, tgt.log_prob, True)
    out = h.transition(mc._point_to(start, dtype), 1, BETA, c["noise_p"].to(dtype), c["noise_e"].to(dtype))
    return out, h, start


@functools.lru_cache(maxsize=None)
def t_case(D, K, nodes, B, n_mix):
    """Everything the tests need of one transition case, in the layout of hmc_mass_cases.case (its `check` applies)."""
    c = t_inputs(D, K, nodes, B, n_mix)
    lw_in = (oais.intermediate_log_prob(c["start"], BETA, ALPHA, False) - c["start"].log_q).detach()
    o64, h64, _ = run_oracle(D, K, nodes, B, n_mix, torch.float64)
    o32, h32, _ = run_oracle(D, K, nodes, B, n_mix, torch.float32)
    band = mc.band_of(o64)
    margins = torch.stack([t["margin"] for t in h64.trace])
    in_band = (margins.abs() <= band).any(0)
    return dict(c, lw_in=lw_in, o64=o64, o32=o32, h64=h64, h32=h32, lw64=mc.log_w_after(o64, lw_in),
                lw32=mc.log_w_after(o32, lw_in.float()), cls64=mc.final_class(h64.trace), cls32=mc.final_class(h32.trace),
                accept=[t["accept"] for t in h64.trace], margins=margins, band=band, in_band=in_band, cap=int(in_band.sum()),
                p_accept=[float(t["p_accept"]) for t in h64.trace])


def perturbed_worst(D, K, nodes, B, n_mix, reps=8, ulps=16):
    """per chain: the worst distance in x, grad_log_p and (at 5e-4, not on the spline flow) grad_log_q (tolerance units) between the float32 and the float64 oracle when BOTH start from the
    case's start moved by up to `ulps` float32 ulps per coordinate - what a kernel that sums a W-long dot product in another order
    does to a pre-activation.  A chain that a ReLU kink, an overflowing proposal or an accept threshold lets jump under such a
    nudge says nothing about the kernel under test; the cases are chosen so that no chain does."""
    c = t_inputs(D, K, nodes, B, n_mix)
    g = torch.Generator().manual_seed(4321 + D + B)
    worst = torch.zeros(B, dtype=torch.float64)
    for _ in range(reps):
        x = (c["start"].x * (1 + ulps * mc.EPS32 / 2 * (2 * torch.rand(B, D, generator=g, dtype=torch.float64) - 1))).float().double()
        start = oais.create_point(x, c["nf64"].log_prob, c["st64"].log_prob, True)
        outs = []
        for dtype in (torch.float32, torch.float64):
            nf = c["nf64"] if dtype == torch.float64 else c["nf"]
            h = oais.HMC(1, D, nf.log_prob, c["make"](dtype).log_prob, alpha=ALPHA, p_target=False, epsilon=c["epsilon"],
                         n_outer=N_OUTER, L=c["L"], eval_mode=True, dtype=dtype)
            h.epsilons, h.common_epsilon = c["eps"].to(dtype).clone(), c["ceps"].to(dtype).clone()
            outs.append(h.transition(mc._point_to(start, dtype), 1, BETA, c["noise_p"].to(dtype), c["noise_e"].to(dtype)))
        worst = torch.maximum(worst, mc.tol_units(outs[0].x, outs[1].x))
        worst = torch.maximum(worst, mc.tol_units(outs[0].grad_log_p, outs[1].grad_log_p))
        if K != mc.SPLINE:                                    # (a knot: grad_log_q is not compared on the spline route)
            worst = torch.maximum(worst, mc.tol_units(outs[0].grad_log_q, outs[1].grad_log_q, 5e-4))
    return worst


def moved_chains(out, start, c, factor=100.0):
    """chains of a mutant's result more than `factor` tolerances from the float64 oracle in x, in log p or in the log-weight
    increment (the mutant's own start point enters its increment, as it would on the device)"""
    lw_in = (oais.intermediate_log_prob(start, BETA, ALPHA, False) - start.log_q).detach()
    inc, inc64 = mc.log_w_after(out, lw_in) - c["lw_in"], c["lw64"] - c["lw_in"]
    return (mc.tol_units(out.x, c["o64"].x) > factor) | (mc.tol_units(inc, inc64) > factor) | \
        (mc.tol_units(out.log_p, c["o64"].log_p) > factor)


# ---- the Metropolis case ----------------------------------------------------------------------------------------------------------
N_UPDATES = 2


@functools.lru_cache(maxsize=None)
def metropolis_case():
    D, K, nodes, B, n_mix = METROPOLIS_SHAPE
    c = t_inputs(D, K, nodes, B, n_mix)
    seed, step, _ = T_PARAMS[(D, K, nodes)]
    g = torch.Generator().manual_seed(7300 + seed)
    noise_x = torch.randn(N_UPDATES, B, D, generator=g)
    noise_u = torch.rand(N_UPDATES, B, generator=g)
    start = oais.Point(c["start"].x, c["start"].log_q, c["start"].log_p)
    lw_in = (oais.intermediate_log_prob(start, BETA, ALPHA, False) - start.log_q).detach()

    def run(dtype, cls=GMMStatement):
        nf = c["nf64"] if dtype == torch.float64 else c["nf"]
        tgt = cls(c["locs"], c["scales"], dtype)
        op = oais.Metropolis(1, D, nf.log_prob, tgt.log_prob, N_UPDATES, alpha=ALPHA, p_target=False, max_step_size=step,
                             min_step_size=step / 2, eval_mode=True, dtype=dtype)
        fresh = lambda: oais.Point(*(t.to(dtype).clone() for t in (start.x, start.log_q, start.log_p)))     # noqa: E731
        out = op.transition(fresh(), 1, BETA, noise_x.to(dtype), noise_u.to(dtype))
        # the same updates once more, keeping every decision and its margin log(acc) - log(u) (metropolis.py:51-74, incl. the
        # acceptance quantity of the START point that is never refreshed)
        cur, accepts, margins = fresh(), [], []
        prev = oais.intermediate_log_prob(cur, BETA, ALPHA, False)
        for n in range(N_UPDATES):
            prop = oais.create_point(cur.x + noise_x[n].to(dtype) * op.noise_scalings[0, n], nf.log_prob, tgt.log_prob, with_grad=False)
            m = (oais.intermediate_log_prob(prop, BETA, ALPHA, False) - prev) - torch.log(noise_u[n].to(dtype))
            accepts.append(m > 0)
            margins.append(m)
            cur[accepts[-1]] = prop[accepts[-1]]
        assert torch.equal(cur.x, out.x)
        return out, torch.stack(accepts), torch.stack(margins)
    o64, acc64, margins = run(torch.float64)
    o32, acc32, _ = run(torch.float32)
    in_band = (margins.abs() <= mc.band_of(o64)).any(0)
    return dict(c, noise_x=noise_x, noise_u=noise_u, start3=start, lw_in=lw_in, o64=o64, o32=o32, run=run, step=step,
                acc64=acc64, acc32=acc32, margins=margins, in_band=in_band, cap=int(in_band.sum()),
                lw64=mc.log_w_after(o64, lw_in), lw32=mc.log_w_after(o32, lw_in.float()))


# ---- whole calls: M_CHAIN transitions, free-running -------------------------------------------------------------------------------
M_CHAIN = mc.M_CHAIN
CHAIN_SHAPES = [(32, 10, 10, 37, 40), (60, 2, 4, 20, 50)]
MIX_SHAPE = (32, 10, 10, 37, 40)
CHAIN_EPS = {(32, 10, 10, False): 0.2, (60, 2, 4, False): 0.3, (32, 10, 10, True): 0.35}
CHAIN_SEED = {(32, 10, 10, False): 2, (60, 2, 4, False): 5, (32, 10, 10, True): 2}


@functools.lru_cache(maxsize=None)
def chain_case(D, K, nodes, B, n_mix, mix=False):
    """oracle.ais.AIS over M_CHAIN transitions with the case's GMM, step sizes frozen, in float64 and float32 (the layout of
    hmc_mass_cases.chain_case: test_gpu_hmc_mass.check_chain applies); `mix`: over defensive_spec's mixture."""
    import defensive_spec as dspec
    c = t_inputs(D, K, nodes, B, n_mix, "call")
    g = torch.Generator().manual_seed(8100 + 97 * CHAIN_SEED[(D, K, nodes, mix)] + D + K)
    eps0 = torch.randn(B, D, generator=g)
    na = torch.randn(M_CHAIN, N_OUTER, B, D, generator=g)
    nb = torch.empty(M_CHAIN, N_OUTER, B).exponential_(generator=g)
    sel = torch.where(torch.arange(B) % 4 == 3, torch.tensor(0.9), torch.tensor(0.2))
    epsilon = CHAIN_EPS[(D, K, nodes, mix)]
    proto = oais.HMC(M_CHAIN, D, None, None, alpha=ALPHA, epsilon=epsilon, n_outer=N_OUTER, L=c["L"])

    def run(dtype):
        nf = c["nf64"] if dtype == torch.float64 else c["nf"]
        tgt = c["st64"] if dtype == torch.float64 else c["st32"]
        base = dspec.DefensiveMixture(nf, torch.full((D,), mc.MIX_LOC, dtype=dtype), torch.full((D,), mc.MIX_LOG_SCALE, dtype=dtype),
                                      mc.MIX_LOGIT) if mix else nf
        h = mc.TraceHMC(M_CHAIN, D, base.log_prob, tgt.log_prob, alpha=ALPHA, p_target=False, epsilon=epsilon, n_outer=N_OUTER,
                        L=c["L"], eval_mode=True, dtype=dtype)
        if mix:
            ais = dspec.make_ais(base, tgt.log_prob, h, False, ALPHA, M_CHAIN, sel.to(dtype))
        else:
            ais = oais.AIS(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, tgt.log_prob, h, False, ALPHA, M_CHAIN)
        pt, lw, info = ais.sample_and_log_weights(eps0.to(dtype), na.to(dtype), nb.to(dtype), keep_snapshots=True)
        assert pt.x.shape[0] == B
        return pt, lw, h, ais.snapshots
    pt64, lw64, h64, snaps = run(torch.float64)
    pt32, lw32, h32, _ = run(torch.float32)
    in_band = torch.zeros(B, dtype=torch.bool)
    margins, bands = [], []
    for j, tr in enumerate(h64.traces):
        band = mc.band_of(snaps[j + 1][0])
        for t in tr:
            in_band |= t["margin"].abs() <= band
            margins.append(t["margin"]); bands.append(band)
    dec64 = torch.stack([t["accept"] for tr in h64.traces for t in tr])
    dec32 = torch.stack([t["accept"] for tr in h32.traces for t in tr])
    return dict(c, margins=torch.stack(margins), bands=torch.stack(bands), epsilon=epsilon, eps=proto.epsilons.clone(),
                ceps=proto.common_epsilon.clone(), eps0=eps0, na=na, nb=nb, sel=sel, pt64=pt64, lw64=lw64, pt32=pt32, lw32=lw32,
                dec64=dec64, dec32=dec32, in_band=in_band, cap=int(in_band.sum()))
