"""Cases for HMC with a non-unit mass vector and an ACTIVE gradient clamp (test_hmc_mass_cases.py asserts every claim made here
from the oracle alone; test_gpu_hmc_mass.py runs the HIP routes on them) - TEST INFRASTRUCTURE, CPU only.

The reference's convention (fab/sampling_methods/transition_operators/hmc.py:126-142, 194-199), which a unit mass cannot tell
from any other:  p0 = noise * m (the mass, not its root);  x += eps / m * p;  K = sum(p^2 / m) / 2;
grad U = nan_to_num(clamp(g, -max_grad, max_grad)): +-inf -> +-max_grad (the clamp sees them first), NaN -> 0.

One case = one seeded flow (test_gpu_parity.seeded_flow's recipe), ManyWell(D), a start Point computed in float64 at
float32-representable x, momentum / exponential noise for N_OUTER = 2 outer steps, and
  * a mass vector, log-uniform in [0.3, 3], every component distinct and mass[j] != mass[j + 16] (the tiled kernels read
    mass[c], mass[c + 16], ...: a lane-indexed read must show); the scalar variant is mass_init = 2.5 passed as a float;
  * max_grad chosen from the float64 oracle's trajectory with the clamp out of reach: the smaller of the 88 % quantile and minus
    the 12 % quantile of every grad U component it evaluated, rounded to float32 - so that the clamp binds on both sides and
    most components stay free (`clamp_shares` counts it on the clamped run by wrapping `_grad_U`);
  * three special rows whose start grad_log_p holds +inf, -inf and NaN at one coordinate each (one of them >= 16 where D allows);
    their exponential noise is SPECIAL_NOISE_E, so that they accept unless the proposal loses more than that: a rejected row
    would return to its start and show nothing of its first half step.
"""
import functools
import math

import numpy as np
import torch

from helpers import RTOL, seeded_oracle_flow
from oracle import ais as oais
from oracle import targets as otgt

N_OUTER, ALPHA, BETA, BETA_NEXT = 2, 2.0, 0.25, 0.5    # beta = 0.25, alpha = 2: log q and log p enter with 0.5 each
EPS32 = 1.1920929e-07
SCALAR_MASS = 2.5
SPECIAL_NOISE_E = 50.0
SPECIAL_ROWS = (1, 5, 11)                               # +inf, -inf, NaN

# (D, K, nodes, B): D < 16 (idle lanes) | two coordinates per lane, W = 512 | the headline width (4- and 8-chain fused stages) |
# D > 32 (16-chain route only, four coordinates per lane) | D < 16 on the 8-chain kernel (W = 240; from
# test_small_tiles_match_sixteen_chain_tiles: (6, 3, 8) has W = 48, below the 8-chain kernel's widths 193 .. 320)
SHAPES = [(6, 3, 8, 37), (32, 2, 16, 37), (32, 10, 10, 37), (60, 2, 4, 20), (6, 2, 40, 37)]
# FABHIP_OPT_TILE_SHAPE values for which a kernel of that tile exists at the shape (16 always does)
TILES = {(6, 3, 8): (16, 4), (32, 2, 16): (16,), (32, 10, 10): (16, 4, 8), (60, 2, 4): (16,), (6, 2, 40): (16, 4, 8)}
# per shape: (seed, step size, leapfrogs).  Seeds and step sizes are chosen so that the conditions of test_hmc_mass_cases.py
# hold (acceptance in [25 %, 90 %], at most one row inside the rounding band, every mutant visible) - from the oracle alone.
# (At D = 6 the kinetic-energy mutants, which change decisions only, need the longer trajectories to flip a quarter of the chains.)
PARAMS = {(6, 3, 8): (3, 0.15, 8), (32, 2, 16): (0, 0.2, 3), (32, 10, 10): (2, 0.2, 3), (60, 2, 4): (0, 0.15, 3),
          (6, 2, 40): (3, 0.2, 5), (20, "plugin", 0): (0, 0.45, 3), (60, "spline", 0): (3, 0.08, 3)}
# the generic path's plug-ins at D = 20 (not a multiple of 16: k_gen_leap_pre reads mass[i % D]) and the spline flow at D = 60
EXTRA_SHAPES = [(20, "plugin", 0, 24), (60, "spline", 0, 20)]


def special_coords(D):
    """coordinates of the +inf, -inf and NaN entries: one below 16, one >= 16 where D allows, the last coordinate."""
    return (1, 17 if D > 17 else D - 2, D - 1)


def mass_vector(D, seed):
    """float32 [D], log-uniform in [0.3, 3], all distinct, mass[j] != mass[j + 16]."""
    g = torch.Generator().manual_seed(9000 + seed)
    m = torch.exp(torch.empty(D, dtype=torch.float64).uniform_(math.log(0.3), math.log(3.0), generator=g)).float()
    assert len(set(m.tolist())) == D and all(m[j] != m[j + 16] for j in range(D - 16))
    return m


class CountingHMC(oais.HMC):
    """oracle HMC that keeps every grad U it evaluated (after the clamp) and, per outer step of the last transition, the
    decision, its margin, the acceptance rate and the proposal: `trace` = [dict(accept, margin, p_accept, x, log_q, log_p)]."""

    def transition(self, *a, **k):
        self.grads, self.trace = [], []
        return super().transition(*a, **k)

    def _outer_step_done(self, proposal):
        self.trace.append(dict(accept=self.last_accept, margin=self.last_margin, p_accept=self.last_p_accept,
                               x=proposal.x.detach().clone(), log_q=proposal.log_q.detach().clone(),
                               log_p=proposal.log_p.detach().clone()))

    def _grad_U(self, pt, beta):
        g = super()._grad_U(pt, beta)
        self.grads.append(g.detach().clone())
        return g


def clamp_shares(h):
    """(share at +max_grad, share at -max_grad, share strictly inside) over every grad U evaluation of h's last transition."""
    g = torch.cat([t.reshape(-1) for t in h.grads])
    mg = h.max_grad
    return float((g == mg).double().mean()), float((g == -mg).double().mean()), float((g.abs() < mg).double().mean())


# ---- mutants: the float64 oracle with ONE line changed ---------------------------------------------------------------------------
class SqrtMassMomentum(oais.HMC):
    def _momentum(self, noise):
        return noise * torch.sqrt(self.mass_vector)


class PositionWithoutMass(oais.HMC):
    def _position(self, x, eps, p):
        return x + eps * p


class KineticWithoutMass(oais.HMC):
    def _kinetic(self, p):
        return torch.sum(p ** 2, -1) / 2


class KineticTimesMass(oais.HMC):
    def _kinetic(self, p):
        return torch.sum(p ** 2 * self.mass_vector, -1) / 2


class LaneIndexedMass(oais.HMC):
    """mass[j % 16] everywhere: what a tiled kernel reading mass[c] for the coordinates c, c + 16, ... computes."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.mass_vector = self.mass_vector[torch.arange(self.dim) % 16]


class ClampAtDefault(oais.HMC):
    def _grad_U(self, pt, beta):
        g = -oais.grad_intermediate_log_prob(pt, beta, self.alpha, self.p_target)
        return torch.nan_to_num(torch.clamp(g, max=1e3, min=-1e3), nan=0.0, posinf=0.0, neginf=0.0)


class InfToZero(oais.HMC):
    def _grad_U(self, pt, beta):
        g = -oais.grad_intermediate_log_prob(pt, beta, self.alpha, self.p_target)
        g = torch.nan_to_num(g, nan=0.0, posinf=0.0, neginf=0.0)
        return torch.clamp(g, max=self.max_grad, min=-self.max_grad)


# name -> (class, rows it must move: "quarter" of all chains or the "special" rows, applies to this D)
MUTANTS = {
    "p0 = noise * sqrt(m)": (SqrtMassMomentum, "quarter", lambda D: True),
    "x += eps * p": (PositionWithoutMass, "quarter", lambda D: True),
    "K = sum(p^2) / 2": (KineticWithoutMass, "quarter", lambda D: True),
    "K = sum(p^2 * m) / 2": (KineticTimesMass, "quarter", lambda D: True),
    "mass[j % 16]": (LaneIndexedMass, "quarter", lambda D: D > 16),          # (the same vector for D <= 16)
    "max_grad = 1e3": (ClampAtDefault, "quarter", lambda D: True),
    "inf -> 0": (InfToZero, "special", lambda D: True),
}


def _point_to(pt, dtype):
    return oais.Point(*(t.to(dtype).clone() for t in (pt.x, pt.log_q, pt.log_p, pt.grad_log_q, pt.grad_log_p)))


def log_w_after(out, lw_in):
    """ais.py:93-100 on the transition's result."""
    return lw_in + (oais.intermediate_log_prob(out, BETA_NEXT, ALPHA, False) - oais.intermediate_log_prob(out, BETA, ALPHA, False))


def final_class(trace):
    """per row: 0 = back at the start, 1 = the first outer step's proposal, 2 = the second's."""
    a0, a1 = trace[0]["accept"], trace[1]["accept"]
    return torch.where(a1, torch.full_like(a1, 2, dtype=torch.long), a0.long())


class PlugGaussian:
    """N(0, scale^2 I) written with tensor expressions: a `Distribution`-style plug-in for the generic path, any device / dtype."""

    def __init__(self, D, scale=2.0):
        self.D, self.scale = D, scale

    def log_prob(self, x):
        return -0.5 * torch.sum((x / self.scale) ** 2, -1) - self.D * (math.log(self.scale) + 0.5 * math.log(2 * math.pi))


class PlugMixture:
    """equal-weight mixture of unit Gaussians at seeded centres: a `LogProbFunc` plug-in (not one of the package's targets)."""

    def __init__(self, D, n=4, spread=1.5, seed=0):
        self.locs = (torch.rand(n, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5) * 2 * spread

    def to(self, device=None, dtype=None):
        m = PlugMixture.__new__(PlugMixture)
        m.locs = self.locs.to(device=device, dtype=dtype)
        return m

    def log_prob(self, x):
        d2 = ((x[:, None, :] - self.locs.to(x.dtype)[None]) ** 2).sum(-1)
        return torch.logsumexp(-0.5 * d2, 1) - math.log(self.locs.shape[0]) - 0.5 * x.shape[1] * math.log(2 * math.pi)


PLUGIN, SPLINE = "plugin", "spline"              # K of a case that is not a RealNVP: the generic path's plug-ins / the spline flow
# (the 60-D set-up of test_gpu_spline.test_hmc_transitions_with_the_spline_flow_on_a_60d_target_vs_oracle)
SPLINE_ARGS = dict(L=12, hidden=256, circ=(3, 7, 8, 12, 20, 21, 22, 30, 41, 45, 52, 59), seed=9, std=0.2)


def spline_pair(D):
    """(float32 oracle spline flow, its float64 copy): test_gpu_spline.make_pair's recipe."""
    import copy
    from oracle import spline as osp
    a = SPLINE_ARGS
    tb = torch.full((D,), 5.0)
    g = torch.Generator().manual_seed(a["seed"])
    tb[list(a["circ"])] = math.pi / (0.5 + torch.rand(len(a["circ"]), generator=g))
    torch.manual_seed(a["seed"])
    of = osp.make_circular_coupled_flow(D, a["L"], a["hidden"], a["circ"], tb, seed=a["seed"])
    osp.randomize(of, a["std"], a["seed"] + 1)
    return of, copy.deepcopy(of).double(), tb


@functools.lru_cache(maxsize=None)
def inputs(D, K, nodes, B):
    """densities (float32 / float64), float64 start point (special rows injected), its un-injected copy, noise, vector mass,
    max_grad.  K = PLUGIN / SPLINE: the plug-in pair of the generic path / the spline flow in place of a RealNVP."""
    import copy
    seed, eps, L = PARAMS[(D, K, nodes)]
    g = torch.Generator().manual_seed(7000 + seed + D + (K if isinstance(K, int) else len(K)))
    eps0 = torch.randn(B, D, generator=g)
    noise_p = torch.randn(N_OUTER, B, D, generator=g)
    noise_e = torch.empty(N_OUTER, B).exponential_(generator=g)
    noise_e[:, list(SPECIAL_ROWS)] = SPECIAL_NOISE_E
    extra = {}
    if K == PLUGIN:
        nf = nf64 = PlugGaussian(D)
        tgt = PlugMixture(D, seed=seed)
        x = (nf.scale * 0.5 * eps0.double()).float().double()
    elif K == SPLINE:
        nf, nf64, tb = spline_pair(D)
        tgt = otgt.ManyWell(D)
        u = torch.rand(B, D, generator=g)
        with torch.no_grad():
            x = nf64.sample_eps(u.double(), eps0.double())[0].float().double()
        extra = dict(tail_bound=tb)
    else:
        nf = seeded_oracle_flow(D, K, nodes, 500 + seed + D + K)
        nf64 = copy.deepcopy(nf).double()
        tgt = otgt.ManyWell(D)
        with torch.no_grad():
            x = nf64.sample_eps(eps0.double())[0].float().double()                 # float32-representable
    plain = oais.create_point(x, nf64.log_prob, tgt.log_prob, True)
    start = plain.clone()
    for r, j, v in zip(SPECIAL_ROWS, special_coords(D), (float("inf"), -float("inf"), float("nan"))):
        start.grad_log_p[r, j] = v
    mass = mass_vector(D, seed + D)
    proto = oais.HMC(1, D, None, None, alpha=ALPHA, epsilon=eps, n_outer=N_OUTER, L=L)   # the step sizes as float32 holds them
    # max_grad: from the float64 trajectory with the clamp out of reach
    free = CountingHMC(1, D, nf64.log_prob, tgt.log_prob, alpha=ALPHA, p_target=False, epsilon=eps, n_outer=N_OUTER, L=L,
                       mass_init=mass.double(), max_grad=1e30, eval_mode=True, dtype=torch.float64)
    free.epsilons, free.common_epsilon = proto.epsilons.double().clone(), proto.common_epsilon.double().clone()
    free.transition(plain.clone(), 1, BETA, noise_p.double(), noise_e.double())
    gall = torch.cat([t.reshape(-1) for t in free.grads])
    gall = gall[torch.isfinite(gall)]
    max_grad = float(np.float32(min(float(torch.quantile(gall, 0.88)), -float(torch.quantile(gall, 0.12)))))
    assert max_grad > 0
    return dict(nf=nf, nf64=nf64, tgt=tgt, start=start, plain=plain, noise_p=noise_p, noise_e=noise_e, mass=mass, max_grad=max_grad,
                eps=proto.epsilons.clone(), ceps=proto.common_epsilon.clone(), L=L, epsilon=eps, eps0=eps0, **extra)


def run_oracle(D, K, nodes, B, mass, dtype=torch.float64, cls=CountingHMC, tune=False, target_p_accept=0.65, start=None,
               max_grad=None):
    """One transition (N_OUTER outer steps) of `cls` from the case's start point; returns (result Point, the operator)."""
    c = inputs(D, K, nodes, B)
    nf = c["nf64"] if dtype == torch.float64 else c["nf"]
    m = mass.to(dtype) if torch.is_tensor(mass) else float(mass)
    h = cls(1, D, nf.log_prob, c["tgt"].log_prob, alpha=ALPHA, p_target=False, epsilon=c["epsilon"], n_outer=N_OUTER, L=c["L"],
            mass_init=m, max_grad=c["max_grad"] if max_grad is None else max_grad, target_p_accept=target_p_accept,
            eval_mode=not tune, dtype=dtype)
    h.epsilons, h.common_epsilon = c["eps"].to(dtype).clone(), c["ceps"].to(dtype).clone()
    out = h.transition(_point_to(c["start"] if start is None else start, dtype), 1, BETA, c["noise_p"].to(dtype), c["noise_e"].to(dtype))
    return out, h


def band_of(o64):
    """the rounding band of test_gpu_stressed_flow.py's transition around a zero margin, per row."""
    return 64 * EPS32 * 3 * (o64.log_q.abs() + o64.log_p.abs()).clamp(min=1.0)


@functools.lru_cache(maxsize=None)
def case(D, K, nodes, B, kind="vector"):
    """Everything the tests need of one case, computed once and never modified.  kind: "vector" or "scalar" mass."""
    c = inputs(D, K, nodes, B)
    mass = c["mass"] if kind == "vector" else SCALAR_MASS
    lw_in = (oais.intermediate_log_prob(c["plain"], BETA, ALPHA, False) - c["plain"].log_q).detach()
    o64, h64 = run_oracle(D, K, nodes, B, mass, torch.float64)
    o32, h32 = run_oracle(D, K, nodes, B, mass, torch.float32)
    band = band_of(o64)
    margins = torch.stack([t["margin"] for t in h64.trace])                                   # [N_OUTER, B] float64
    in_band = (margins.abs() <= band).any(0)
    return dict(c, kind=kind, mass_init=mass, lw_in=lw_in, o64=o64, o32=o32, h64=h64, h32=h32, lw64=log_w_after(o64, lw_in),
                lw32=log_w_after(o32, lw_in.float()), cls64=final_class(h64.trace), cls32=final_class(h32.trace),
                accept=[t["accept"] for t in h64.trace], margins=margins, band=band, in_band=in_band, cap=int(in_band.sum()),
                shares=clamp_shares(h64), p_accept=[float(t["p_accept"]) for t in h64.trace])


# (D, K, nodes, B, tile shape) of the step-size tests: one shape per tile size, the headline width on both small tiles
TUNED = [(60, 2, 4, 20, 16), (6, 3, 8, 37, 4), (32, 10, 10, 37, 8), (32, 10, 10, 37, 4)]
TARGET_LOW, TARGET_HIGH = 0.05, 0.95      # target_p_accept below / above every acceptance rate of the cases: both branches of the rule


@functools.lru_cache(maxsize=None)
def tuned(D, K, nodes, B, kind, target, dtype=torch.float32):
    """The case's transition with step-size tuning ON (the second outer step runs on the common step size the first one
    adapted): result, adapted step sizes, final classes, acceptance rates, rows inside the rounding band."""
    c = inputs(D, K, nodes, B)
    out, h = run_oracle(D, K, nodes, B, c["mass"] if kind == "vector" else SCALAR_MASS, dtype, tune=True, target_p_accept=target)
    margins = torch.stack([t["margin"] for t in h.trace]).double()
    in_band = (margins.abs() <= band_of(out).double()).any(0)
    return dict(out=out, epsilons=h.epsilons.clone(), ceps=h.common_epsilon.clone(), cls=final_class(h.trace),
                p_accept=[float(t["p_accept"]) for t in h.trace], in_band=in_band, cap=int(in_band.sum()), trace=h.trace)


def tol_units(a, b, rtol=RTOL):
    """per row: the worst element of |a - b| in units of the tolerance of helpers.close at `rtol` (scale of the whole tensor b)."""
    a, b = a.detach().double(), b.detach().double()
    fin = torch.isfinite(b)
    scale = max(1.0, float(b[fin].abs().max()))
    u = (a - b).abs() / (rtol * b.abs() + 2e-6 * scale)
    u = torch.where(fin, u, torch.zeros_like(u))
    return u.reshape(u.shape[0], -1).amax(1)


def moved_rows(out, lw, c, factor=100.0):
    """rows of a mutant's result more than `factor` tolerances from the float64 oracle in x or in the log-weight increment."""
    inc, inc64 = lw - c["lw_in"], c["lw64"] - c["lw_in"]
    return (tol_units(out.x, c["o64"].x) > factor) | (tol_units(inc, inc64) > factor)


def all_cases():
    return [(D, K, nodes, B, kind) for D, K, nodes, B in SHAPES for kind in ("vector", "scalar")] + \
        [s + ("vector",) for s in EXTRA_SHAPES]


# ---- the whole fused call: M_CHAIN transitions, free-running ---------------------------------------------------------------------
M_CHAIN = 3
MIX_LOC, MIX_LOG_SCALE, MIX_LOGIT = 0.0, 0.3, 1.0
CHAIN_SHAPES = [(32, 10, 10, 37), (60, 2, 4, 20)]            # tile shapes 4 / 8 / 16, and the 16-chain route alone
MIX_SHAPE = (32, 10, 10, 37)                                 # k_hmc_step_mix (16-chain tiles) over the defensive mixture


class TraceHMC(CountingHMC):
    """keeps the trace and the grad U evaluations of EVERY transition of a call."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.traces, self.all_grads = [], []

    def transition(self, *a, **k):
        out = super().transition(*a, **k)
        self.traces.append(self.trace)
        self.all_grads += self.grads
        return out


# (D, K, nodes, mix) -> step size of the whole call: three free-running transitions compound float32 rounding, and at the
# headline depth the float32 ORACLE leaves M x the tolerance at the single transition's step size (test_hmc_mass_cases.py)
CHAIN_EPS = {(32, 10, 10, False): 0.1, (60, 2, 4, False): 0.15, (32, 10, 10, True): 0.2}
CHAIN_SEED = {(32, 10, 10, False): 4, (60, 2, 4, False): 0, (32, 10, 10, True): 3}     # (D, K, nodes, mix) -> noise seed


def chain_noise(D, K, nodes, B, n_outer=N_OUTER, mix=False):
    g = torch.Generator().manual_seed(8000 + 97 * CHAIN_SEED[(D, K, nodes, mix)] + D + K + n_outer)
    eps0 = torch.randn(B, D, generator=g)
    na = torch.randn(M_CHAIN, n_outer, B, D, generator=g)
    nb = torch.empty(M_CHAIN, n_outer, B).exponential_(generator=g)
    sel = torch.where(torch.arange(B) % 4 == 3, torch.tensor(0.9), torch.tensor(0.2))     # far from sigmoid(1) = 0.731 on both sides
    return eps0, na, nb, sel


@functools.lru_cache(maxsize=None)
def chain_case(D, K, nodes, B, mix=False):
    """oracle.ais.AIS over M_CHAIN transitions with the case's vector mass and max_grad, step sizes frozen, in float64 and float32;
    with `mix` the base distribution is defensive_spec's mixture around the same flow (its transition takes the HMC unchanged)."""
    import defensive_spec as dspec
    c = inputs(D, K, nodes, B)
    eps0, na, nb, sel = chain_noise(D, K, nodes, B, mix=mix)
    epsilon = CHAIN_EPS[(D, K, nodes, mix)]
    proto = oais.HMC(M_CHAIN, D, None, None, alpha=ALPHA, epsilon=epsilon, n_outer=N_OUTER, L=c["L"])

    def run(dtype):
        nf = c["nf64"] if dtype == torch.float64 else c["nf"]
        base = dspec.DefensiveMixture(nf, torch.full((D,), MIX_LOC, dtype=dtype), torch.full((D,), MIX_LOG_SCALE, dtype=dtype),
                                      MIX_LOGIT) if mix else nf
        h = TraceHMC(M_CHAIN, D, base.log_prob, c["tgt"].log_prob, alpha=ALPHA, p_target=False, epsilon=epsilon,
                     n_outer=N_OUTER, L=c["L"], mass_init=c["mass"].to(dtype), max_grad=c["max_grad"], eval_mode=True, dtype=dtype)
        if mix:
            ais = dspec.make_ais(base, c["tgt"].log_prob, h, False, ALPHA, M_CHAIN, sel.to(dtype))
        else:
            ais = oais.AIS(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, c["tgt"].log_prob, h, False, ALPHA,
                           M_CHAIN)
        pt, lw, info = ais.sample_and_log_weights(eps0.to(dtype), na.to(dtype), nb.to(dtype), keep_snapshots=True)
        assert pt.x.shape[0] == B
        return pt, lw, h, ais.snapshots
    pt64, lw64, h64, snaps = run(torch.float64)
    pt32, lw32, h32, _ = run(torch.float32)
    in_band = torch.zeros(B, dtype=torch.bool)
    margins, bands = [], []
    for j, tr in enumerate(h64.traces):
        band = band_of(snaps[j + 1][0])
        for t in tr:
            in_band |= t["margin"].abs() <= band
            margins.append(t["margin"]); bands.append(band)
    dec64 = torch.stack([t["accept"] for tr in h64.traces for t in tr])            # [M_CHAIN * N_OUTER, B]
    dec32 = torch.stack([t["accept"] for tr in h32.traces for t in tr])
    h64.grads = h64.all_grads
    return dict(c, margins=torch.stack(margins), bands=torch.stack(bands), epsilon=epsilon, eps=proto.epsilons.clone(), ceps=proto.common_epsilon.clone(), eps0=eps0, na=na, nb=nb, sel=sel, pt64=pt64, lw64=lw64, pt32=pt32, lw32=lw32, dec64=dec64, dec32=dec32,
                in_band=in_band, cap=int(in_band.sum()), shares=clamp_shares(h64))
