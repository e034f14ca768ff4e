"""The coupled-rotor target (FABHIP_TARGET_ROTOR, csrc/target_device.h) - its DEFINITION, its cases and their conditions
(test_rotor_cases.py asserts every claim made here on the CPU; test_gpu_rotor.py runs the HIP routes on the cases) - TEST
INFRASTRUCTURE, CPU only.  The reference has no such target: as with quartic_cases.py the specification lives here.

    t_j = x_j r_j          w_j = t_j - rint(t_j)          theta_j = 2 pi w_j            (revolutions first: the reduction is exact)
    d_jn = (w_j - w_k) - rint(w_j - w_k),  k = k_jn

    log p(x)       = sum_j [ sum_{m=1..3} (A_mj cos(m theta_j) + B_mj sin(m theta_j)) - l_j x_j - q_j x_j^2 ]
                     + 1/2 sum_j sum_{n<NB} kap_jn cos(2 pi d_jn)  -  log_norm
    d log p / dx_j = 2 pi r_j [ sum_m m (-A_mj sin(m theta_j) + B_mj cos(m theta_j)) - sum_n kap_jn sin(2 pi d_jn) ] - l_j - 2 q_j x_j

r_j = 1 / P_j for a periodic site of period P_j, 0 for a site on the line.  The neighbour table (indices k_jn, couplings kap_jn,
width NB) is the row form of a symmetric coupling K with a zero diagonal that is non-zero between periodic sites only: every bond is
listed from both ends (that makes the gradient line above correct), a site's neighbours in ascending k, unused slots padded with
k = j, kap = 0, NB = max(1, largest row count).  `neighbour_table` builds it here as the class does in the package.

The layout is the C ABI's: `rows` = [9][D] (A1 A2 A3 B1 B2 B3 r l q), `table` = [2 NB][D] (rows 0 .. NB - 1 the indices as floats,
rows NB .. 2 NB - 1 the couplings).

RESTATEMENT.  `RotorStatement` writes both lines out in float64 or float32 with every place a wrong factor or index could sit as
a one-line method; a mutant overrides one line.  Sine and cosine are evaluated as the kernel evaluates them - from the reduced
revolutions, by quarter turns (q = rint(4 w) in -2 .. 2, the remainder's sine and cosine, the quadrant put back) - so that an
argument that was NOT reduced a second time shows: in float64 the remainder's sine and cosine are torch's, in float32 the kernel's
polynomials, and w_j = fma(x_j, r_j, -rint(x_j r_j)) keeps the low bits of the product.  Harmonics 2 and 3 come from the
angle-addition recurrence.  The float32 form sums as the kernel does: the neighbour sums in ascending n; lane c of a row owns
the sites c, c + 16, c + 32, c + 48 and adds their energies in that order; the 16 lanes are added as a rotation tree (8, 4, 2, 1).  Non-finite coordinates propagate through these very operations (inf r -> rint -> NaN;
0 inf = NaN on a line site): there is no mask.

DIRECT CASES.  D in DIMS, per D a SPARSE and a nearly DENSE coupling (up to 44 neighbours at D = 64), a random mix of periodic
and line sites (all periodic for D <= 2), periods in [2, 7], |A|, |B| <= 1, l in [-0.5, 0.5], q in [0.2, 1.5], K of magnitude
0.5 / sqrt(NB); B_ROWS rows (periodic coordinates uniform in [-1.5 P, 1.5 P], line coordinates in [-3, 3]) and four special rows
(a NaN coordinate, +inf on a periodic site, +inf on a line site, all zeros); log_norm = LOG_NORM.

TRANSITION CASES.  The seeded flows of hmc_mass_cases.SHAPES (and its plug-in / spline shapes, a Metropolis case at D = 5, whole
calls of M = 3) with a rotor target drawn the same way but gentler (harmonic m within T_AMPLITUDE / m^2, couplings of magnitude
T_AMPLITUDE / sqrt(NB), periods in T_PERIODS: the direct cases' Fourier rows have curvatures of up to (2 pi / 2)^2 x 14, far too
stiff for a leapfrog step that the flows' own scale allows); on the spline shape the periodic sites
are the flow's circular coordinates with period 2 tail_bound.  Unit mass, max_grad = 1e3; (seed, step size, leapfrogs) per shape
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
DENSITIES = ("sparse", "dense")
INF = float("inf")
LOG_NORM = 3.25            # of every direct case: a constant no property hands out (its sign is one of the one-line places)
N_SITE_ROWS = 9
ROW_RATE, ROW_L, ROW_Q = 6, 7, 8


def neighbour_table(K):
    """[2 NB, D] float64 from a symmetric K with a zero diagonal: rows 0 .. NB - 1 the neighbour indices (ascending k, padded with
    k = j), rows NB .. 2 NB - 1 the couplings (padded with 0)"""
    D = K.shape[0]
    assert torch.equal(K, K.T) and bool((torch.diagonal(K) == 0).all())
    lists = [[k for k in range(D) if K[j, k] != 0] for j in range(D)]
    NB = max(1, max(len(v) for v in lists))
    idx = torch.arange(D, dtype=torch.float64)[None].repeat(NB, 1)
    kap = torch.zeros(NB, D, dtype=torch.float64)
    for j, v in enumerate(lists):
        for n, k in enumerate(v):
            idx[n, j], kap[n, j] = k, K[j, k]
    return torch.cat([idx, kap])


class RotorStatement(tc._Statement):
    def __init__(self, rows, table, dtype=torch.float64, log_norm=0.0):
        self.dim = D = rows.shape[1]
        assert rows.shape == (N_SITE_ROWS, D) and table.dim() == 2 and table.shape[1] == D and table.shape[0] % 2 == 0
        self.NB = table.shape[0] // 2
        self.rows, self.table, self.dtype, self.log_norm = rows.to(dtype), table.to(dtype), dtype, log_norm

    # ---- the one-line places -----------------------------------------------------------------------------------------------
    def _coupling_energy_factor(self):
        return 0.5

    def _angle_gradient_factor(self, r):
        return 2.0 * math.pi * r

    def _harmonic_multiplier(self, m):
        return float(m)

    def _sine_gradient_sign(self):
        return -1.0

    def _coupling_row_offset(self):
        """couplings sit NB rows below the indices"""
        return self.NB

    def _table_row(self, r):
        """the D floats the lanes read of table row r: T[r * D + j], j = 0 .. D - 1"""
        return self.table.reshape(-1)[r * self.dim: r * self.dim + self.dim]

    def _normalise(self, lp):
        return lp - self.log_norm

    def _reduce_difference(self, d):
        return d - torch.round(d)

    # -----------------------------------------------------------------------------------------------------------------------
    def _sincos(self, w):
        """(sin, cos) of 2 pi w for w in [-1/2, 1/2], by quarter turns as the kernel's sincos_rev"""
        y = 4.0 * w
        q = torch.round(y)
        a = (y - q) * (math.pi / 2)
        if self.dtype == torch.float64:
            ps, pc = torch.sin(a), torch.cos(a)
        else:
            a2 = a * a
            ps = torch.full_like(a, 2.7557319223985893e-6)
            for c in (-1.9841269841269841e-4, 8.3333333333333333e-3, -1.6666666666666667e-1):
                ps = ps * a2 + c
            ps = a + a * (a2 * ps)
            pc = torch.full_like(a, 2.4801587301587302e-5)
            for c in (-1.3888888888888889e-3, 4.1666666666666667e-2, -0.5):
                pc = pc * a2 + c
            pc = 1.0 + a2 * pc
        odd = q.abs() == 1
        two = q.abs() == 2
        ss, cc = torch.where(odd, pc, ps), torch.where(odd, ps, pc)
        return torch.where((q == -1) | two, -ss, ss), torch.where((q == 1) | two, -cc, cc)

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

    def revolutions(self, x):
        r = self.rows[ROW_RATE]
        n = torch.round(x * r)
        if self.dtype == torch.float64:
            return x * r - n
        return (x.double() * r.double() - n.double()).float()      # the kernel's fmaf(x, r, -n): x r - n rounded once

    def log_prob_and_grad(self, x):
        x = x.to(self.dtype)
        A, Bc = self.rows[0:3], self.rows[3:6]
        r, l, q = self.rows[ROW_RATE], self.rows[ROW_L], self.rows[ROW_Q]
        w = self.revolutions(x)
        ce, cg = torch.zeros_like(x), torch.zeros_like(x)
        for n in range(self.NB):                               # ascending n
            k = self._table_row(n).long().clamp(0, self.dim - 1)
            kap = self._table_row(self._coupling_row_offset() + n)
            d = self._reduce_difference(w - w[:, k])
            sd, cd = self._sincos(d)
            ce = ce + kap * cd
            cg = cg + kap * sd
        s1, c1 = self._sincos(w)
        c2, s2 = c1 * c1 - s1 * s1, 2.0 * (s1 * c1)
        c3, s3 = c2 * c1 - s2 * s1, s2 * c1 + c2 * s1
        e = (A[0] * c1 + Bc[0] * s1) + (A[1] * c2 + Bc[1] * s2) + (A[2] * c3 + Bc[2] * s3) - l * x - q * (x * x) \
            + self._coupling_energy_factor() * ce
        sg = self._sine_gradient_sign()
        gs = (Bc[0] * c1 + sg * A[0] * s1) + self._harmonic_multiplier(2) * (Bc[1] * c2 + sg * A[1] * s2) \
            + self._harmonic_multiplier(3) * (Bc[2] * c3 + sg * A[2] * s3)
        g = self._angle_gradient_factor(r) * (gs - cg) - l - 2.0 * q * x
        return self._normalise(self._row_sum(e)), g


def plain_log_prob(rows, K, x, log_norm=0.0):
    """the first line of the definition written once more in float64 with torch's own cos / sin of 2 pi x r and the coupling as
    a matrix (no table, no reduction: the density is periodic)"""
    rows, K, x = rows.double(), K.double(), x.double()
    th = 2.0 * math.pi * x * rows[ROW_RATE]
    lp = -(rows[ROW_L] * x + rows[ROW_Q] * x * x).sum(-1)
    for m in (1, 2, 3):
        lp = lp + (rows[m - 1] * torch.cos(m * th) + rows[2 + m] * torch.sin(m * th)).sum(-1)
    lp = lp + 0.5 * (K[None] * torch.cos(th[:, :, None] - th[:, None, :])).sum((1, 2))
    return lp - log_norm


# ---- mutants: the statement with ONE line changed ----------------------------------------------------------------------------------
class CouplingEnergyWithoutHalf(RotorStatement):
    def _coupling_energy_factor(self):
        return 1.0


class AngleGradientWithoutRate(RotorStatement):
    """2 pi for 2 pi r_j"""

    def _angle_gradient_factor(self, r):
        return 2.0 * math.pi * (r > 0).to(r.dtype)


class AngleGradientWithoutTwoPi(RotorStatement):
    def _angle_gradient_factor(self, r):
        return r


class HarmonicsWithoutMultiplier(RotorStatement):
    def _harmonic_multiplier(self, m):
        return 1.0


class HarmonicThreeTimesTwo(RotorStatement):
    def _harmonic_multiplier(self, m):
        return 2.0


class SineGradientPlus(RotorStatement):
    def _sine_gradient_sign(self):
        return 1.0


class CouplingRowsOneAbove(RotorStatement):
    """couplings read NB - 1 rows below the indices: the first one is the last row of indices"""

    def _coupling_row_offset(self):
        return self.NB - 1


class TableStrideSixteen(RotorStatement):
    """T[r * 16 + j]: the lane count in place of D (reads wrap inside the buffer)"""

    def _table_row(self, r):
        n = self.table.numel()
        return self.table.reshape(-1)[(r * 16 + torch.arange(self.dim)) % n]


class LogNormAdded(RotorStatement):
    def _normalise(self, lp):
        return lp + self.log_norm


class DifferenceNotReducedAgain(RotorStatement):
    def _reduce_difference(self, d):
        return d


# name -> (class, where it shows: "both" / "log_p" / "grad", can differ at D)
MUTANTS = {
    "coupling energy without its 1/2": (CouplingEnergyWithoutHalf, "log_p", lambda D: D > 1),
    "2 pi for 2 pi r in the gradient": (AngleGradientWithoutRate, "grad", lambda D: True),
    "r for 2 pi r in the gradient": (AngleGradientWithoutTwoPi, "grad", lambda D: True),
    "harmonics 2 and 3 without their multipliers": (HarmonicsWithoutMultiplier, "grad", lambda D: True),
    "2 for 3 on the third harmonic": (HarmonicThreeTimesTwo, "grad", lambda D: True),
    "+ A sin in the gradient": (SineGradientPlus, "grad", lambda D: True),
    "couplings read NB - 1 rows below the indices": (CouplingRowsOneAbove, "both", lambda D: D > 1),
    "table read with stride 16": (TableStrideSixteen, "both", lambda D: D not in (1, 16)),
    "+ log_norm": (LogNormAdded, "log_p", lambda D: True),
    # (D = 2 is one bond: its difference leaves [-1/2, 1/2] on a quarter of the rows only - too few for "a quarter of the rows")
    "d not reduced a second time": (DifferenceNotReducedAgain, "both", lambda D: D > 2),
}


# ---- direct cases ------------------------------------------------------------------------------------------------------------------
def draw_sites(D, g, periodic=None, amplitude=1.0, periods=None, period_range=(2.0, 7.0), decay=0):
    """float64 (P [D] with 0 on line sites, A [3, D], B [3, D], l [D], q [D]); `periodic`: the mask (drawn at 3 / 4 when None, all
    periodic for D <= 2); `periods`: given periods of the periodic sites (drawn in `period_range` when None); harmonic m is drawn
    in +-amplitude / m^decay"""
    u = lambda lo, hi, *shape: torch.empty(*shape, dtype=torch.float64).uniform_(lo, hi, generator=g)       # noqa: E731
    if periodic is None:
        periodic = u(0, 1, D) < 0.75 if D > 2 else torch.ones(D, dtype=torch.bool)
        if D > 2:
            periodic[0], periodic[D - 1] = True, False          # both kinds at every D > 2, a periodic site on lane 0
    P = torch.where(periodic, u(*period_range, D) if periods is None else periods, torch.zeros(D, dtype=torch.float64))
    fall = torch.arange(1.0, 4.0, dtype=torch.float64)[:, None] ** -decay
    A, B = u(-amplitude, amplitude, 3, D) * periodic * fall, u(-amplitude, amplitude, 3, D) * periodic * fall
    l, q = u(-0.5, 0.5, D) * ~periodic, u(0.2, 1.5, D) * ~periodic
    return P, A, B, l, q


def draw_coupling(P, g, density, magnitude=0.5):
    """float64 symmetric K, zero diagonal, non-zero between periodic sites only, entries of magnitude `magnitude` / sqrt(NB) (in
    [0.3, 1] of it, either sign); "sparse": about three neighbours a site, "dense": nine pairs of ten"""
    D = P.shape[0]
    per = P > 0
    n_per = int(per.sum())
    p = 0.9 if density == "dense" else min(1.0, 3.0 / max(n_per - 1, 1))
    U = torch.rand(D, D, generator=g, dtype=torch.float64)
    mask = torch.triu(U < p, 1) & per[:, None] & per[None, :]
    if n_per >= 2 and not bool(mask.any()):
        i = torch.nonzero(per).flatten()
        mask[i[0], i[1]] = True
    mask = mask | mask.T
    NB = max(1, int(mask.sum(1).max()))
    V = torch.empty(D, D, dtype=torch.float64).uniform_(0.3, 1.0, generator=g) * \
        torch.where(torch.rand(D, D, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    V = torch.triu(V, 1)
    return (V + V.T) * mask * (magnitude / math.sqrt(NB))


def pack(P, A, B, l, q, K):
    """float32 (rows [9, D], table [2 NB, D]) as the package stores them, and K as float32 holds it"""
    line = P == 0
    rate = torch.where(line, torch.zeros_like(P), 1.0 / torch.where(line, torch.ones_like(P), P))
    rows = torch.cat([A, B, rate[None], l[None], q[None]]).float()
    K32 = K.float()
    K32 = torch.triu(K32, 1) + torch.triu(K32, 1).T
    return rows, neighbour_table(K32.double()).float(), K32


@functools.lru_cache(maxsize=None)
def case(D, density):
    """dict(P, A, B, l, q, K (float64 as drawn), rows, table, K32 (float32), st64, st32, rows_x {"wide", "special"}: float64 at
    float32-representable values, ref {...})"""
    g = torch.Generator().manual_seed(9700 + 2 * D + DENSITIES.index(density))
    P, A, B, l, q = draw_sites(D, g)
    K = draw_coupling(P, g, density)
    rows, table, K32 = pack(P, A, B, l, q, K)
    st64, st32 = RotorStatement(rows, table, log_norm=LOG_NORM), RotorStatement(rows, table, torch.float32, LOG_NORM)
    per = P > 0
    span = torch.where(per, 1.5 * P, torch.full_like(P, 3.0))
    wide = (2 * torch.rand(B_ROWS, D, generator=g, dtype=torch.float64) - 1) * span
    wide[0, 0], wide[1, D - 1] = span[0], -span[D - 1]
    special = (2 * torch.rand(4, D, generator=g, dtype=torch.float64) - 1) * span
    i_per = torch.nonzero(per).flatten()
    i_line = torch.nonzero(~per).flatten()
    special[0, D // 2] = float("nan")
    special[1, i_per[-1]] = INF
    if len(i_line):
        special[2, i_line[-1]] = INF                            # (D <= 2 has no line site: the row stays an ordinary one)
    special[3] = 0.0
    rows_x = {"wide": wide.float().double(), "special": special.float().double()}
    return dict(D=D, density=density, P=P, A=A, B=B, l=l, q=q, K=K, rows=rows, table=table, K32=K32, NB=table.shape[0] // 2,
                log_norm=LOG_NORM, st64=st64, st32=st32, rows_x=rows_x, has_line=bool(len(i_line)),
                ref={n: st64.log_prob_and_grad(x) for n, x in rows_x.items()})


def all_cases():
    return [(D, d) for D in DIMS for d in DENSITIES]


def lattice_action(shape, coupling, field, period, x):
    """-log p of the XY model, loop-written, float64: -coupling sum_x sum_mu cos(theta_x - theta_(x + mu)) - field sum_x cos theta_x
    over the directions of extent > 1; x: [B, prod(shape)] in row-major site order"""
    f = (x.double() * (2.0 * math.pi / period)).reshape((x.shape[0],) + tuple(shape))
    S = torch.zeros(x.shape[0], dtype=torch.float64)
    for site in np.ndindex(*shape):
        v = f[(slice(None),) + site]
        S -= field * torch.cos(v)
        for mu in range(len(shape)):
            if shape[mu] == 1:
                continue
            nb = list(site)
            nb[mu] = (nb[mu] + 1) % shape[mu]
            S -= coupling * torch.cos(v - f[(slice(None),) + tuple(nb)])
    return S


LATTICES = [(2,), (3,), (2, 2), (4, 4), (2, 3, 2), (8, 8)]


# ---- transition cases --------------------------------------------------------------------------------------------------------------
N_OUTER, ALPHA, BETA, BETA_NEXT = mc.N_OUTER, mc.ALPHA, mc.BETA, mc.BETA_NEXT
T_SHAPES = list(mc.SHAPES)                                    # (D, K, nodes, B)
T_TILES = dict(mc.TILES)
METROPOLIS_SHAPE = (5, 2, 4, 37)
EXTRA_SHAPES = list(mc.EXTRA_SHAPES)                          # the generic path's base / the spline flow
T_AMPLITUDE, T_PERIODS = 0.3, (4.0, 7.0)
T_PERTURB_REPS = {(32, 10, 10): 16}                           # repetitions of perturbed_worst per shape (4 elsewhere)
# per shape: (seed, step size, leapfrogs), chosen from the float64 oracle so that the conditions of test_rotor_cases.py hold
# ((32, 10, 10): T_PERTURB_REPS asks for 16 repetitions of perturbed_worst in place of 4 - the flow is ten layers deep and a chain
# near a ReLU kink shows only under more nudges: the oracle's worst distance is 10 tolerances at seed 0, 49 at seed 1 and 53 at seed
# 2 (seeds 1 and 2 stay at 0.08 under 4 repetitions), 0.07 at seed 3, the first seed that meets every condition)
T_PARAMS = {(6, 3, 8): (1, 0.5, 3), (32, 2, 16): (0, 0.3, 3), (32, 10, 10): (3, 0.25, 3), (60, 2, 4): (2, 0.3, 3),
            (6, 2, 40): (1, 0.4, 3), (5, 2, 4): (0, 0.8, 2), (20, "plugin", 0): (2, 0.4, 3), (60, "spline", 0): (6, 0.03, 3),
            ("call", 32, 10, 10): (0, 0.25, 3), ("call", 60, 2, 4): (0, 0.3, 3)}
CHAIN_SHAPES = list(mc.CHAIN_SHAPES)
MIX_SHAPE = mc.MIX_SHAPE
CHAIN_EPS = {(32, 10, 10, False): 0.105, (60, 2, 4, False): 0.2, (32, 10, 10, True): 0.2}
CHAIN_SEED = {(32, 10, 10, False): 5, (60, 2, 4, False): 0, (32, 10, 10, True): 0}
M_CHAIN = mc.M_CHAIN
N_UPDATES = 2


@functools.lru_cache(maxsize=None)
def t_inputs(D, K, nodes, B, variant=None):
    """flow (float32 / float64), rotor statement pair, float64 start point at a sample of the flow, noise"""
    seed, eps, L = T_PARAMS[(variant, D, K, nodes) if variant else (D, K, nodes)]
    g = torch.Generator().manual_seed(9800 + seed + D + (K if isinstance(K, int) else len(K)))
    eps0 = torch.randn(B, D, generator=g)
    noise_p = torch.randn(N_OUTER, B, D, generator=g)
    noise_e = torch.empty(N_OUTER, B).exponential_(generator=g)
    extra, periodic, periods = {}, None, None
    if K == mc.PLUGIN:
        nf = nf64 = mc.PlugGaussian(D)
        x = (nf.scale * 0.5 * eps0.double()).float().double()
    elif K == mc.SPLINE:
        nf, nf64, tb = mc.spline_pair(D)
        u = torch.rand(B, D, generator=g)
        with torch.no_grad():
            x = nf64.sample_eps(u.double(), eps0.double())[0].float().double()
        extra = dict(tail_bound=tb)
        periodic = torch.zeros(D, dtype=torch.bool)
        periodic[list(mc.SPLINE_ARGS["circ"])] = True           # the flow's torus: period 2 tail_bound on its circular coordinates
        periods = 2.0 * tb.double()
    else:
        nf = seeded_oracle_flow(D, K, nodes, 700 + seed + D + K)
        nf64 = copy.deepcopy(nf).double()
        with torch.no_grad():
            x = nf64.sample_eps(eps0.double())[0].float().double()                 # float32-representable
    P, A, Bs, l, q = draw_sites(D, g, periodic=periodic, amplitude=T_AMPLITUDE, periods=periods, period_range=T_PERIODS, decay=2)
    Kc = draw_coupling(P, g, "sparse" if D > 8 else "dense", T_AMPLITUDE)
    rows, table, K32 = pack(P, A, Bs, l, q, Kc)
    make = lambda dtype, cls=RotorStatement: cls(rows, table, dtype)               # noqa: E731
    st64, st32 = make(torch.float64), make(torch.float32)
    start = oais.create_point(x, nf64.log_prob, st64.log_prob, True)
    proto = oais.HMC(1, D, None, None, alpha=ALPHA, epsilon=eps, n_outer=N_OUTER, L=L)     # the step sizes as float32 holds them
    return dict(nf=nf, nf64=nf64, P=P, A=A, B=Bs, l=l, q=q, K=Kc, rows=rows, table=table, K32=K32, st64=st64, st32=st32,
                start=start, noise_p=noise_p, noise_e=noise_e, eps=proto.epsilons.clone(), ceps=proto.common_epsilon.clone(), L=L,
                epsilon=eps, eps0=eps0, mass=torch.ones(D), max_grad=1e3, make=make, **extra)


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


def nudged(x, g, ulps=16):
    """the rows moved by up to `ulps` float32 ulps per coordinate, float32-representable again"""
    return (x * (1 + ulps * mc.EPS32 / 2 * (2 * torch.rand(x.shape, generator=g, dtype=torch.float64) - 1))).float().double()


def perturbed_worst(D, K, nodes, B, reps=None, ulps=16):
    """per chain: the worst distance in x and grad_log_p (tolerance units) between the float32 and the float64 oracle when both
    start from the case's start moved by up to `ulps` float32 ulps per coordinate (target_cases.perturbed_worst)"""
    c = t_inputs(D, K, nodes, B)
    g = torch.Generator().manual_seed(4321 + D + B)
    worst = torch.zeros(B, dtype=torch.float64)
    for _ in range(T_PERTURB_REPS.get((D, K, nodes), 4) if reps is None else reps):
        start = oais.create_point(nudged(c["start"].x, g, ulps), c["nf64"].log_prob, c["st64"].log_prob, True)
        outs = [run_oracle(D, K, nodes, B, dtype, start=start)[0] for dtype in (torch.float32, torch.float64)]
        worst = torch.maximum(worst, mc.tol_units(outs[0].x, outs[1].x))
        worst = torch.maximum(worst, mc.tol_units(outs[0].grad_log_p, outs[1].grad_log_p))
    return worst


def moved_chains(out, start, c, factor=100.0):
    return tc.moved_chains(out, start, c, factor)


@functools.lru_cache(maxsize=None)
def metropolis_case():
    """target_cases.metropolis_case with the rotor target"""
    D, K, nodes, B = METROPOLIS_SHAPE
    c = t_inputs(D, K, nodes, B)
    seed, step, _ = T_PARAMS[(D, K, nodes)]
    g = torch.Generator().manual_seed(9900 + seed)
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
    """oracle.ais.AIS over M_CHAIN transitions with the case's rotor target, step sizes frozen, float64 and float32 (the layout
    of hmc_mass_cases.chain_case: test_gpu_hmc_mass.check_chain applies); `mix`: over defensive_spec's mixture."""
    import defensive_spec as dspec
    c = t_inputs(D, K, nodes, B, "call")
    g = torch.Generator().manual_seed(9950 + 97 * CHAIN_SEED[(D, K, nodes, mix)] + D + K)
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
