"""The coupled-quartic target (FABHIP_TARGET_QUARTIC, csrc/target_device.h) - its DEFINITION, its cases and their conditions
(test_quartic_cases.py asserts every claim made here on the CPU; test_gpu_quartic.py runs the HIP routes on the cases) - TEST
INFRASTRUCTURE, CPU only.  The reference has no such target: as with smc_spec.py and defensive_spec.py the specification lives here.

    log p(x)       = - sum_j (a_j x_j + b_j x_j^2 + c_j x_j^4)  -  1/2 sum_j x_j (J x)_j  -  log_norm        J symmetric [D, D]
    d log p / dx_j = -(a_j + 2 b_j x_j + 4 c_j x_j^3) - (J x)_j

RESTATEMENT.  `QuarticStatement` writes both out in float64 or float32 with every place a wrong factor or index could sit as a
one-line method; a mutant overrides one line.  The float32 form sums as the kernel does: (J x)_j = sum_k J[k][j] x_k in ascending
k; lane c of a row owns the sites c, c + 16, c + 32, c + 48 and adds their energies in that order; the 16 lanes are added as a
rotation tree (8, 4, 2, 1).

DIRECT CASES.  D in DIMS (ragged against the 16-lane site mapping on both sides), a DENSE random symmetric J (a stencil would
let a stride error read zeros for zeros), distinct site coefficients, B_ROWS rows uniform in [-3, 3] and three special rows
(one NaN coordinate, one +inf coordinate, all zeros), log_norm = LOG_NORM.  The coefficients are scaled (c in [0.05, 0.3], |a| <= 0.5, b in [-1.5, 0.5],
J_jk ~ 0.3 N(0, 1) / sqrt(D)) so that the float32 statement stays inside `helpers.close` of the float64 one on these rows.

TRANSITION CASES.  The seeded flows of hmc_mass_cases.SHAPES (and its plug-in / spline shapes, a Metropolis case at D = 5, whole
calls of M = 3) with a quartic target drawn the same way; unit mass, max_grad = 1e3; (seed, step size, leapfrogs) per shape
chosen from the oracle alone so that no accept decision sits inside the rounding band and the float32 oracle takes the float64
oracle's decisions.
"""
import copy
import functools
import math

import numpy as np
import torch

import hmc_mass_cases as mc
import target_cases as tc
from helpers import seeded_oracle_flow
from oracle import ais as oais

B_ROWS = 48
DIMS = (1, 2, 15, 16, 17, 33, 64)
INF = float("inf")
LOG_NORM = 3.25            # of every direct case: a constant no property hands out (its sign is one of the one-line places)


class QuarticStatement(tc._Statement):
    def __init__(self, a, b, c, J, dtype=torch.float64, log_norm=0.0):
        self.dim = D = a.shape[0]
        assert a.shape == b.shape == c.shape == (D,) and J.shape == (D, D)
        self.a, self.b, self.c, self.J, self.dtype, self.log_norm = a.to(dtype), b.to(dtype), c.to(dtype), J.to(dtype), dtype, log_norm

    # ---- the one-line places -----------------------------------------------------------------------------------------------
    def _coupling_energy_factor(self):
        return 0.5

    def _coupling_gradient_factor(self):
        return 1.0

    def _quadratic_gradient_factor(self):
        return 2.0

    def _quartic_gradient_factor(self):
        return 4.0

    def _J_row(self, k):
        """the D floats the lanes read for x_k: J[k * D + j], j = 0 .. D - 1"""
        return self.J.reshape(-1)[k * self.dim: k * self.dim + self.dim]

    def _site_rows(self):
        """rows a, b, c of the [3][D] site coefficients"""
        return self.a, self.b, self.c

    def _sites_summed(self, e):
        return e

    def _normalise(self, lp):
        return lp - self.log_norm

    # -----------------------------------------------------------------------------------------------------------------------
    def _row_sum(self, e):
        """sum over the sites: plain in float64, in the kernel's order in float32"""
        if self.dtype == torch.float64:
            return e.sum(-1)
        B, D = e.shape
        pad = torch.zeros(B, 64, dtype=e.dtype)
        pad[:, :D] = e
        lanes = pad.view(B, 4, 16)
        v = torch.zeros(B, 16, dtype=e.dtype)
        for s in range(4):
            v = v + lanes[:, s]
        for w in (8, 4, 2, 1):
            v = v[:, :w] + v[:, w:]
        return v[:, 0]

    def jx(self, x):
        out = torch.zeros_like(x)
        for k in range(self.dim):                              # ascending k
            out = out + self._J_row(k)[None, :] * x[:, k:k + 1]
        return out

    def log_prob_and_grad(self, x):
        x = x.to(self.dtype)
        a, b, c = self._site_rows()
        jx = self.jx(x)
        x2 = x * x
        e = a * x + b * x2 + c * (x2 * x2) + self._coupling_energy_factor() * x * jx
        lp = self._row_sum(self._sites_summed(-e))
        g = -(a + self._quadratic_gradient_factor() * b * x + self._quartic_gradient_factor() * c * (x2 * x)) \
            - self._coupling_gradient_factor() * jx
        return self._normalise(lp), g


# ---- mutants: the statement with ONE line changed ----------------------------------------------------------------------------------
class CouplingEnergyWithoutHalf(QuarticStatement):
    def _coupling_energy_factor(self):
        return 1.0


class CouplingGradientWithHalf(QuarticStatement):
    def _coupling_gradient_factor(self):
        return 0.5


class QuadraticGradientWithoutTwo(QuarticStatement):
    def _quadratic_gradient_factor(self):
        return 1.0


class QuarticGradientWithoutFour(QuarticStatement):
    def _quartic_gradient_factor(self):
        return 1.0


class CouplingStrideSixteen(QuarticStatement):
    """J[k * 16 + j]: the lane count in place of D (reads wrap inside the buffer)"""

    def _J_row(self, k):
        n = self.dim * self.dim
        return self.J.reshape(-1)[(k * 16 + torch.arange(self.dim)) % n]


class CouplingStrideOneMore(QuarticStatement):
    """J[k * (D + 1) + j]"""

    def _J_row(self, k):
        n = self.dim * self.dim
        return self.J.reshape(-1)[(k * (self.dim + 1) + torch.arange(self.dim)) % n]


class SiteRowsBAndCSwapped(QuarticStatement):
    def _site_rows(self):
        return self.a, self.c, self.b


class SiteRowsFromRowA(QuarticStatement):
    """row r read at r * (D - 1): a row stride one short"""

    def _site_rows(self):
        flat, D = torch.cat([self.a, self.b, self.c]), self.dim
        return tuple(flat[r * (D - 1): r * (D - 1) + D] for r in range(3))


class SitesBeyondSixteenDropped(QuarticStatement):
    def _sites_summed(self, e):
        return e * (torch.arange(self.dim) < 16).to(e.dtype)


class LogNormAdded(QuarticStatement):
    def _normalise(self, lp):
        return lp + self.log_norm


# name -> (class, where it shows: "both" / "log_p" / "grad", can differ at D)
MUTANTS = {
    "coupling energy without its 1/2": (CouplingEnergyWithoutHalf, "log_p", lambda D: True),
    "coupling gradient with a 1/2": (CouplingGradientWithHalf, "grad", lambda D: True),
    "b for 2 b in the gradient": (QuadraticGradientWithoutTwo, "grad", lambda D: True),
    "c for 4 c in the gradient": (QuarticGradientWithoutFour, "grad", lambda D: True),
    "J read with stride 16": (CouplingStrideSixteen, "both", lambda D: D not in (1, 16)),
    "J read with stride D + 1": (CouplingStrideOneMore, "both", lambda D: D > 1),
    "site rows b and c swapped": (SiteRowsBAndCSwapped, "both", lambda D: True),
    "site rows with stride D - 1": (SiteRowsFromRowA, "both", lambda D: True),
    "sites j >= 16 dropped from log p": (SitesBeyondSixteenDropped, "log_p", lambda D: D > 16),
    "+ log_norm": (LogNormAdded, "log_p", lambda D: True),
}


# ---- direct cases ------------------------------------------------------------------------------------------------------------------
def draw_coefficients(D, g):
    """float32 (a, b, c [D], J [D, D] symmetric and dense), every site coefficient distinct"""
    while True:
        a = torch.empty(D, dtype=torch.float64).uniform_(-0.5, 0.5, generator=g).float()
        b = torch.empty(D, dtype=torch.float64).uniform_(-1.5, 0.5, generator=g).float()
        c = torch.empty(D, dtype=torch.float64).uniform_(0.05, 0.3, generator=g).float()
        if len(set(torch.cat([a, b, c]).tolist())) == 3 * D:
            break
    R = torch.randn(D, D, generator=g, dtype=torch.float64) * (0.3 / math.sqrt(D))
    J = ((R + R.T) / math.sqrt(2.0)).float()
    J = torch.triu(J) + torch.triu(J, 1).T                      # symmetric in its float32 bits
    assert torch.equal(J, J.T) and bool((J != 0).all())
    return a, b, c, J


@functools.lru_cache(maxsize=None)
def case(D):
    """dict(a, b, c, J (float32), st64, st32, rows {"wide", "special"}: float64 at float32-representable values, ref {...})"""
    g = torch.Generator().manual_seed(9000 + D)
    a, b, c, J = draw_coefficients(D, g)
    st64, st32 = QuarticStatement(a, b, c, J, log_norm=LOG_NORM), QuarticStatement(a, b, c, J, torch.float32, LOG_NORM)
    wide = torch.empty(B_ROWS, D, dtype=torch.float64).uniform_(-3.0, 3.0, generator=g)
    wide[0, 0], wide[1, D - 1] = 3.0, -3.0
    special = torch.empty(3, D, dtype=torch.float64).uniform_(-2.0, 2.0, generator=g)
    special[0, D // 2] = float("nan")
    special[1, D - 1] = INF
    special[2] = 0.0
    rows = {"wide": wide.float().double(), "special": special.float().double()}
    return dict(D=D, a=a, b=b, c=c, J=J, log_norm=LOG_NORM, st64=st64, st32=st32, rows=rows, ref={n: st64.log_prob_and_grad(x) for n, x in rows.items()})


def nudged(x, g, ulps=16):
    """the rows moved by up to `ulps` float32 ulps per coordinate, float32-representable again"""
    return (x * (1 + ulps * mc.EPS32 / 2 * (2 * torch.rand(x.shape, generator=g, dtype=torch.float64) - 1))).float().double()


def manywell_form(D, abc=tc.DEFAULT_ABC):
    """(a, b, c, J) of ManyWell(D) in this family: even sites (a, b, c), odd sites b = 1/2, a = c = 0; no coupling"""
    even = (torch.arange(D) % 2 == 0).double()
    return abc[0] * even, abc[1] * even + 0.5 * (1 - even), abc[2] * even, torch.zeros(D, D, dtype=torch.float64)


def lattice_action(shape, kappa, lam, phi):
    """S = sum_x [(1 - 2 lam) phi_x^2 + lam phi_x^4] - 2 kappa sum_x sum_mu phi_x phi_(x + mu), loop-written, float64;
    phi: [B, prod(shape)] in row-major site order"""
    f = phi.double().reshape((phi.shape[0],) + tuple(shape))
    S = torch.zeros(phi.shape[0], dtype=torch.float64)
    for site in np.ndindex(*shape):
        v = f[(slice(None),) + site]
        S += (1 - 2 * lam) * v * v + lam * v ** 4
        for mu in range(len(shape)):
            nb = list(site)
            nb[mu] = (nb[mu] + 1) % shape[mu]
            S -= 2 * kappa * v * f[(slice(None),) + tuple(nb)]
    return S


LATTICES = [(2,), (3,), (2, 2), (4, 4), (2, 3, 2), (8, 8)]


# ---- transition cases --------------------------------------------------------------------------------------------------------------
N_OUTER, ALPHA, BETA, BETA_NEXT = mc.N_OUTER, mc.ALPHA, mc.BETA, mc.BETA_NEXT
T_SHAPES = list(mc.SHAPES)                                    # (D, K, nodes, B)
T_TILES = dict(mc.TILES)
METROPOLIS_SHAPE = (5, 2, 4, 37)
EXTRA_SHAPES = list(mc.EXTRA_SHAPES)                          # the generic path's base / the spline flow
# per shape: (seed, step size, leapfrogs), chosen from the float64 oracle so that the conditions of test_quartic_cases.py hold
T_PARAMS = {(6, 3, 8): (0, 0.5, 3), (32, 2, 16): (0, 0.3, 3), (32, 10, 10): (0, 0.25, 3), (60, 2, 4): (0, 0.3, 3),
            (6, 2, 40): (4, 0.4, 3), (5, 2, 4): (0, 0.8, 2), (20, "plugin", 0): (2, 0.4, 3), (60, "spline", 0): (2, 0.03, 3),
            ("call", 32, 10, 10): (0, 0.25, 3), ("call", 60, 2, 4): (0, 0.3, 3)}
CHAIN_SHAPES = list(mc.CHAIN_SHAPES)
MIX_SHAPE = mc.MIX_SHAPE
CHAIN_EPS = {(32, 10, 10, False): 0.105, (60, 2, 4, False): 0.2, (32, 10, 10, True): 0.2}
CHAIN_SEED = {(32, 10, 10, False): 5, (60, 2, 4, False): 2, (32, 10, 10, True): 2}
M_CHAIN = mc.M_CHAIN
N_UPDATES = 2


@functools.lru_cache(maxsize=None)
def t_inputs(D, K, nodes, B, variant=None):
    """flow (float32 / float64), quartic statement pair, float64 start point at a sample of the flow, noise"""
    seed, eps, L = T_PARAMS[(variant, D, K, nodes) if variant else (D, K, nodes)]
    g = torch.Generator().manual_seed(9100 + seed + D + (K if isinstance(K, int) else len(K)))
    eps0 = torch.randn(B, D, generator=g)
    noise_p = torch.randn(N_OUTER, B, D, generator=g)
    noise_e = torch.empty(N_OUTER, B).exponential_(generator=g)
    extra = {}
    if K == mc.PLUGIN:
        nf = nf64 = mc.PlugGaussian(D)
        x = (nf.scale * 0.5 * eps0.double()).float().double()
    elif K == mc.SPLINE:
        nf, nf64, tb = mc.spline_pair(D)
        u = torch.rand(B, D, generator=g)
        with torch.no_grad():
            x = nf64.sample_eps(u.double(), eps0.double())[0].float().double()
        extra = dict(tail_bound=tb)
    else:
        nf = seeded_oracle_flow(D, K, nodes, 700 + seed + D + K)
        nf64 = copy.deepcopy(nf).double()
        with torch.no_grad():
            x = nf64.sample_eps(eps0.double())[0].float().double()                 # float32-representable
    a, b, c, J = draw_coefficients(D, g)
    make = lambda dtype, cls=QuarticStatement: cls(a, b, c, J, dtype)               # noqa: E731
    st64, st32 = make(torch.float64), make(torch.float32)
    start = oais.create_point(x, nf64.log_prob, st64.log_prob, True)
    proto = oais.HMC(1, D, None, None, alpha=ALPHA, epsilon=eps, n_outer=N_OUTER, L=L)     # the step sizes as float32 holds them
    return dict(nf=nf, nf64=nf64, a=a, b=b, c=c, J=J, st64=st64, st32=st32, start=start, noise_p=noise_p, noise_e=noise_e,
                eps=proto.epsilons.clone(), ceps=proto.common_epsilon.clone(), L=L, epsilon=eps, eps0=eps0,
                mass=torch.ones(D), max_grad=1e3, make=make, **extra)


def _hmc(c, D, dtype, target, cls=mc.CountingHMC, n_dist=1, epsilon=None, log_q=None):
    nf = c["nf64"] if dtype == torch.float64 else c["nf"]
    return cls(n_dist, D, nf.log_prob if log_q is None else log_q, target.log_prob, alpha=ALPHA, p_target=False,
               epsilon=c["epsilon"] if epsilon is None else epsilon, n_outer=N_OUTER, L=c["L"], eval_mode=True, dtype=dtype)


def run_oracle(D, K, nodes, B, dtype=torch.float64, target_cls=None, start=None):
    """One transition (N_OUTER outer steps) of the oracle HMC from the case's start point (a mutant: from ITS point)."""
    c = t_inputs(D, K, nodes, B)
    tgt = c["make"](dtype) if target_cls is None else c["make"](dtype, target_cls)
    h = _hmc(c, D, dtype, tgt)
    h.epsilons, h.common_epsilon = c["eps"].to(dtype).clone(), c["ceps"].to(dtype).clone()
    if start is None:
        start = c["start"] if target_cls is None else oais.create_point(c["start"].x, c["nf64"].log_prob, tgt.log_prob, True)
    out = h.transition(mc._point_to(start, dtype), 1, BETA, c["noise_p"].to(dtype), c["noise_e"].to(dtype))
    return out, h, start


@functools.lru_cache(maxsize=None)
def t_case(D, K, nodes, B):
    """Everything the tests need of one transition case, in the layout of hmc_mass_cases.case (test_gpu_hmc_mass.check applies)."""
    c = t_inputs(D, K, nodes, B)
    lw_in = (oais.intermediate_log_prob(c["start"], BETA, ALPHA, False) - c["start"].log_q).detach()
    o64, h64, _ = run_oracle(D, K, nodes, B, torch.float64)
    o32, h32, _ = run_oracle(D, K, nodes, B, torch.float32)
    band = mc.band_of(o64)
    margins = torch.stack([t["margin"] for t in h64.trace])
    in_band = (margins.abs() <= band).any(0)
    return dict(c, lw_in=lw_in, o64=o64, o32=o32, h64=h64, h32=h32, lw64=mc.log_w_after(o64, lw_in),
                lw32=mc.log_w_after(o32, lw_in.float()), cls64=mc.final_class(h64.trace), cls32=mc.final_class(h32.trace),
                accept=[t["accept"] for t in h64.trace], margins=margins, band=band, in_band=in_band, cap=int(in_band.sum()),
                p_accept=[float(t["p_accept"]) for t in h64.trace])


def perturbed_worst(D, K, nodes, B, reps=4, ulps=16):
    """per chain: the worst distance in x and grad_log_p (tolerance units) between the float32 and the float64 oracle when both
    start from the case's start moved by up to `ulps` float32 ulps per coordinate (target_cases.perturbed_worst)"""
    c = t_inputs(D, K, nodes, B)
    g = torch.Generator().manual_seed(4321 + D + B)
    worst = torch.zeros(B, dtype=torch.float64)
    for _ in range(reps):
        start = oais.create_point(nudged(c["start"].x, g, ulps), c["nf64"].log_prob, c["st64"].log_prob, True)
        outs = [run_oracle(D, K, nodes, B, dtype, start=start)[0] for dtype in (torch.float32, torch.float64)]
        worst = torch.maximum(worst, mc.tol_units(outs[0].x, outs[1].x))
        worst = torch.maximum(worst, mc.tol_units(outs[0].grad_log_p, outs[1].grad_log_p))
    return worst


def moved_chains(out, start, c, factor=100.0):
    return tc.moved_chains(out, start, c, factor)


@functools.lru_cache(maxsize=None)
def metropolis_case():
    """target_cases.metropolis_case with the quartic target"""
    D, K, nodes, B = METROPOLIS_SHAPE
    c = t_inputs(D, K, nodes, B)
    seed, step, _ = T_PARAMS[(D, K, nodes)]
    g = torch.Generator().manual_seed(9300 + seed)
    noise_x = torch.randn(N_UPDATES, B, D, generator=g)
    noise_u = torch.rand(N_UPDATES, B, generator=g)
    start = oais.Point(c["start"].x, c["start"].log_q, c["start"].log_p)
    lw_in = (oais.intermediate_log_prob(start, BETA, ALPHA, False) - start.log_q).detach()

    def run(dtype):
        nf = c["nf64"] if dtype == torch.float64 else c["nf"]
        tgt = c["make"](dtype)
        op = oais.Metropolis(1, D, nf.log_prob, tgt.log_prob, N_UPDATES, alpha=ALPHA, p_target=False, max_step_size=step,
                             min_step_size=step / 2, eval_mode=True, dtype=dtype)
        fresh = lambda: oais.Point(*(t.to(dtype).clone() for t in (start.x, start.log_q, start.log_p)))     # noqa: E731
        out = op.transition(fresh(), 1, BETA, noise_x.to(dtype), noise_u.to(dtype))
        cur, margins = fresh(), []
        prev = oais.intermediate_log_prob(cur, BETA, ALPHA, False)
        for n in range(N_UPDATES):
            prop = oais.create_point(cur.x + noise_x[n].to(dtype) * op.noise_scalings[0, n], nf.log_prob, tgt.log_prob, with_grad=False)
            m = (oais.intermediate_log_prob(prop, BETA, ALPHA, False) - prev) - torch.log(noise_u[n].to(dtype))
            margins.append(m)
            cur[m > 0] = prop[m > 0]
        assert torch.equal(cur.x, out.x)
        return out, torch.stack(margins)
    o64, margins = run(torch.float64)
    o32, m32 = run(torch.float32)
    in_band = (margins.abs() <= mc.band_of(o64)).any(0)
    return dict(c, noise_x=noise_x, noise_u=noise_u, start3=start, lw_in=lw_in, o64=o64, o32=o32, step=step,
                acc64=margins > 0, acc32=m32 > 0, margins=margins, in_band=in_band, cap=int(in_band.sum()),
                lw64=mc.log_w_after(o64, lw_in), lw32=mc.log_w_after(o32, lw_in.float()))


@functools.lru_cache(maxsize=None)
def chain_case(D, K, nodes, B, mix=False):
    """oracle.ais.AIS over M_CHAIN transitions with the case's quartic target, step sizes frozen, float64 and float32 (the layout
    of hmc_mass_cases.chain_case: test_gpu_hmc_mass.check_chain applies); `mix`: over defensive_spec's mixture."""
    import defensive_spec as dspec
    c = t_inputs(D, K, nodes, B, "call")
    g = torch.Generator().manual_seed(9500 + 97 * CHAIN_SEED[(D, K, nodes, mix)] + D + K)
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
        h = _hmc(c, D, dtype, tgt, mc.TraceHMC, M_CHAIN, epsilon, base.log_prob)
        if mix:
            ais = dspec.make_ais(base, tgt.log_prob, h, False, ALPHA, M_CHAIN, sel.to(dtype))
        else:
            ais = oais.AIS(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, tgt.log_prob, h, False, ALPHA, M_CHAIN)
        pt, lw, info = ais.sample_and_log_weights(eps0.to(dtype), na.to(dtype), nb.to(dtype), keep_snapshots=True)
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
