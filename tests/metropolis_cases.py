"""Cases for the native Metropolis transition and its noise-scaling rule away from D = 2 (test_metropolis_cases.py asserts every
claim made here from the oracle alone; test_gpu_metropolis.py runs the HIP entries on them) - TEST INFRASTRUCTURE, CPU only.

The reference's transition (metropolis.py:51-74) with the three quirks a kernel has to copy:
  * the acceptance quantity of the START point is computed once and never refreshed (:53);
  * acc = nan_to_num(exp(d), nan = 0, posinf = 0, neginf = 0) BEFORE clamp_max(acc, 1): a proposal whose ratio overflows float32
    is rejected and adds 0 to the mean acceptance;
  * log_w is left alone when beta_next == beta (ais.py:93).
`TraceMetropolis` / `CallAIS` are copies of oracle.ais.Metropolis / AIS with every place a one-line mistake could sit written as
a one-line method (test_metropolis_cases.py pins them to the originals bit for bit), so that a mutant is a one-line override.

One shape per compiled column-tile variant of k_metropolis (padded width / 64 = 1, 2, 4, 5, 8), D < 16, D = 18 (two coordinates
on lanes 0-1 only), D = 32 and D = 60 (four coordinates per lane, not a multiple of 16).  n_updates = 3, beta 0.25 -> 0.5,
alpha = 2; flows from seeded_oracle_flow(std = 0.05) and a float64 deep copy; start points are flow samples; the operator holds
a [2, 3] table of six distinct log-spaced scalings and the transition is number 2 (row 1: a read of row 0 shows).

THE RULE STATEMENT is numpy float32: s * float32(1.05) or s / float32(1.05), the direction from the float64 oracle's p_accept;
a case is admitted only if every |p_accept - target| >= 1e-3 (the float32 sum of at most 37 terms in [0, 1] is nowhere near).
"""
import copy
import functools

import numpy as np
import torch

import hmc_mass_cases as mc
import target_cases as tc
from helpers import seeded_oracle_flow
from oracle import ais as oais
from oracle import numerical as onum
from oracle import targets as otgt

N_UPDATES, ALPHA, BETA, BETA_NEXT, TARGET = 3, mc.ALPHA, mc.BETA, mc.BETA_NEXT, 0.65
TARGET_LOW, TARGET_HIGH = 0.05, 0.95
ADMIT = 1e-3
F105 = np.float32(1.05)
N_MIX = 17
INF = float("inf")

# (D, K, nodes, B): width 48 -> variant 1 | 108 -> 2 | 256 -> 4 | 320 -> 5 (the headline width) | 480 -> 8 (the GMM case)
SHAPES = [(6, 3, 8, 37), (18, 2, 6, 37), (32, 2, 8, 37), (32, 3, 10, 37), (60, 2, 8, 20)]
VARIANT = {(6, 3, 8): 1, (18, 2, 6): 2, (32, 2, 8): 4, (32, 3, 10): 5, (60, 2, 8): 8}
GMM_SHAPES = {(60, 2, 8)}
P_TARGET_SHAPES = [(32, 2, 8, 37), (32, 3, 10, 37)]
# (D, K, nodes, p_target) -> (seed, largest scaling of the transition's row; the smallest is a third of it).  Chosen from the
# float64 oracle so that the conditions of test_metropolis_cases.py hold.
PARAMS = {(6, 3, 8, False): (3, 0.7), (18, 2, 6, False): (5, 0.4), (32, 2, 8, False): (6, 0.35), (32, 3, 10, False): (2, 0.25),
          (60, 2, 8, False): (4, 0.2), (32, 2, 8, True): (6, 0.35), (32, 3, 10, True): (2, 0.25)}
ROW = 2                                     # the transition number of the teacher-forced cases: row 1 of the table


def all_cases():
    return [s + (False,) for s in SHAPES] + [s + (True,) for s in P_TARGET_SHAPES]


def variant_of(width):
    """padded width / 64 of the column-tile variant the dispatcher picks (fabhip_common.h: 1, 2, 4, 5 or 8)"""
    p = -(-width // 64)
    return p if p <= 2 else (4 if p <= 4 else (5 if p <= 5 else 8))


# ---- the reference's transition and call with one-line hooks ------------------------------------------------------------------------
class TraceMetropolis:
    """oracle.ais.Metropolis over a given [n_dist, n_updates] table, keeping per update the decision, its margin
    (log ratio - log u), the acceptance ratio after nan_to_num and the mean the rule saw: `traces[-1]` = the last transition's."""
    uses_grad_info = False

    def __init__(self, table, log_q_fn, log_p_fn, alpha=ALPHA, p_target=False, target_p_accept=TARGET, tune=True):
        self.noise_scalings = table.clone()
        self.n_updates = table.shape[1]
        self.log_q_fn, self.log_p_fn, self.alpha, self.p_target = log_q_fn, log_p_fn, alpha, p_target
        self.target_prob_accept, self.tune = target_p_accept, tune
        self.traces, self.rows = [], None               # rows: the original chain numbers of the rows of a compacted batch

    # ---- the one-line places -----------------------------------------------------------------------------------------------------
    def _density(self, pt, beta):
        return oais.intermediate_log_prob(pt, beta, self.alpha, self.p_target)

    def _scale(self, i, n):
        return self.noise_scalings[i - 1, n]

    def _noise(self, noise, n, B):
        return noise[n, :B]

    def _acc(self, d):
        return torch.nan_to_num(torch.exp(d), nan=0.0, posinf=0.0, neginf=0.0)

    def _prev_after(self, prev, prop_lp, accept):
        return prev

    def _p_accept(self, acc):
        return torch.mean(torch.clamp_max(acc, 1))

    def _grows(self, p_accept):
        return p_accept > self.target_prob_accept

    # -----------------------------------------------------------------------------------------------------------------------------
    def transition(self, point, i, beta, noise_x, noise_u):
        prev = self._density(point, beta)
        trace = []
        for n in range(self.n_updates):
            B = point.x.shape[0]
            x_prop = point.x + self._noise(noise_x, n, B) * self._scale(i, n)
            prop = oais.create_point(x_prop, self.log_q_fn, self.log_p_fn, with_grad=False)
            prop_lp = self._density(prop, beta)
            acc = self._acc(prop_lp - prev)
            u = self._noise(noise_u, n, B)
            accept = acc > u
            point[accept] = prop[accept]
            p_accept = self._p_accept(acc)
            trace.append(dict(accept=accept.clone(), margin=((prop_lp - prev) - torch.log(u)).detach().clone(),
                              log_ratio=(prop_lp - prev).detach().clone(), acc=acc.detach().clone(), p_accept=float(p_accept)))
            prev = self._prev_after(prev, prop_lp, accept)
            if self.tune:
                if self._grows(p_accept):
                    self.noise_scalings[i - 1, n] = self.noise_scalings[i - 1, n] * 1.05
                else:
                    self.noise_scalings[i - 1, n] = self.noise_scalings[i - 1, n] / 1.05
        self.traces.append(trace)
        return point


class PrevRefreshed(TraceMetropolis):
    def _prev_after(self, prev, prop_lp, accept):
        return torch.where(accept, prop_lp, prev)


class ClampBeforeNanToNum(TraceMetropolis):
    def _acc(self, d):
        return torch.nan_to_num(torch.clamp_max(torch.exp(d), 1), nan=0.0, posinf=0.0, neginf=0.0)


class PosinfToOne(TraceMetropolis):
    def _acc(self, d):
        return torch.nan_to_num(torch.exp(d), nan=0.0, posinf=1.0, neginf=0.0)


class NoClampInTheMean(TraceMetropolis):
    def _p_accept(self, acc):
        return torch.mean(acc)


class MeanOverAllocatedRows(TraceMetropolis):
    n_allocated = None

    def _p_accept(self, acc):
        return torch.sum(torch.clamp_max(acc, 1)) / self.n_allocated


class RowZeroForEveryTransition(TraceMetropolis):
    def _scale(self, i, n):
        return self.noise_scalings[0, n]


class ColumnZeroForEveryUpdate(TraceMetropolis):
    def _scale(self, i, n):
        return self.noise_scalings[i - 1, 0]


class RuleInverted(TraceMetropolis):
    def _grows(self, p_accept):
        return not (p_accept > self.target_prob_accept)


class CoefficientsOfTheOtherTarget(TraceMetropolis):
    def _density(self, pt, beta):
        return oais.intermediate_log_prob(pt, beta, ALPHA, not self.p_target)


class NoiseByOriginalChainNumber(TraceMetropolis):
    def _noise(self, noise, n, B):
        return noise[n, self.rows]


class CallAIS(oais.AIS):
    """oracle.ais.AIS.sample_and_log_weights with the log-weight step as one-line methods; also returns the survivors' original
    chain numbers (`kept`) and hands them to the operator (`rows`)."""

    def _log_w_moves(self, j):
        return self.B_space[j + 1] != self.B_space[j]

    def _increment(self, point, before, j):
        return oais.intermediate_log_prob(point, self.B_space[j + 1], self.alpha, self.p_target) - \
            oais.intermediate_log_prob(point, self.B_space[j], self.alpha, self.p_target)

    def sample_and_log_weights(self, eps0, noise_a, noise_b, keep_snapshots=False):
        batch_size = eps0.shape[0]
        x, log_q0 = self.sample_eps_fn(eps0)
        point = oais.create_point(x, self.log_q_fn, self.log_p_fn, with_grad=False, log_q_x=log_q0)
        log_w = (oais.intermediate_log_prob(point, self.B_space[1], self.alpha, self.p_target) - log_q0).detach()
        valid = torch.isfinite(point.log_p) & torch.isfinite(point.log_q)
        point, log_w = oais.remove_nan_and_infs(point, log_w, "chain init")
        self.kept = valid.nonzero().flatten()
        self.transition_operator.rows = self.kept
        with torch.no_grad():
            ess_base = onum.effective_sample_size(point.log_p - point.log_q).item()
        self.snapshots = [(point.clone(), log_w.clone())]
        for j in range(1, self.M + 1):
            before = point.clone()
            point = self.transition_operator.transition(point, j, self.B_space[j], noise_a[j - 1], noise_b[j - 1])
            if self._log_w_moves(j):
                log_w = log_w + self._increment(point, before, j)
            self.snapshots.append((point.clone(), log_w.clone()))
        point, log_w = oais.remove_nan_and_infs(point, log_w, "chain end")
        with torch.no_grad():
            ess_ais = onum.effective_sample_size(log_w).item()
            lz = torch.logsumexp(log_w, dim=0)
            log_Z = (lz - torch.log(torch.ones_like(lz) * batch_size)).item()
        return point, log_w.detach(), oais.LoggingInfo(ess_base, ess_ais, log_Z)


class LogWMovesWhenBetaRepeats(CallAIS):
    def _log_w_moves(self, j):
        return True


class IncrementFromTheStartPoint(CallAIS):
    def _increment(self, point, before, j):
        return super()._increment(before, before, j)


# ---- the rule statement ---------------------------------------------------------------------------------------------------------------
def rule_statement(scalings, grows):
    """numpy float32: s * float32(1.05) where the mean acceptance lay above the target, s / float32(1.05) where not"""
    s = np.asarray(scalings, dtype=np.float32)
    g = np.asarray(grows, dtype=bool)
    assert s.shape == g.shape
    return np.where(g, s * F105, s / F105).astype(np.float32)


def directions(p_accept, target):
    """per update: does the scaling grow - and the case's admission: no mean acceptance within ADMIT of the target"""
    p = np.asarray(p_accept, dtype=np.float64)
    assert bool((np.abs(p - target) >= ADMIT).all()), f"a mean acceptance within {ADMIT} of the target {target}: {p.tolist()}"
    return p > target


def scaling_table(step, n_dist=2, n_updates=N_UPDATES):
    """float32 [n_dist, n_updates], every entry distinct: the LAST row log-spaced from `step` down to a third of it, the rows in
    front of it the same values in reverse order, scaled by 0.83, 0.83^2, ..."""
    last = step * 3.0 ** (-torch.arange(n_updates, dtype=torch.float64) / max(1, n_updates - 1))
    rows = [last.flip(0) * 0.83 ** (n_dist - 1 - r) if r < n_dist - 1 else last for r in range(n_dist)]
    t = torch.stack(rows).float()
    assert len(set(t.reshape(-1).tolist())) == t.numel()
    return t


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flow_pair(D, K, nodes, seed):
    nf = seeded_oracle_flow(D, K, nodes, 700 + seed + D + K, std=0.05)
    return nf, copy.deepcopy(nf).double()


@functools.lru_cache(maxsize=None)
def target_pair(D, K, nodes, seed):
    """(float32, float64) target of the shape: ManyWell, or at D = 60 a 17-component GMM with its means at samples of the flow
    and target_cases' per-entry scales.  Third entry: (locs, scales) or None."""
    if (D, K, nodes) not in GMM_SHAPES:
        t = otgt.ManyWell(D)
        return t, t, None
    _, nf64 = flow_pair(D, K, nodes, seed)
    g = torch.Generator().manual_seed(7500 + seed + D)
    with torch.no_grad():
        locs = nf64.sample_eps(torch.randn(N_MIX, D, generator=g).double())[0].float()
    scales = tc.draw_scales(N_MIX, D, 950 + seed + D)
    return tc.GMMStatement(locs, scales, torch.float32), tc.GMMStatement(locs, scales, torch.float64), (locs, scales)


def _point3(pt, dtype, rows=slice(None)):
    return oais.Point(*(t[rows].to(dtype).clone() for t in (pt.x, pt.log_q, pt.log_p)))


@functools.lru_cache(maxsize=None)
def inputs(D, K, nodes, B, p_target=False):
    seed, step = PARAMS[(D, K, nodes, p_target)]
    nf, nf64 = flow_pair(D, K, nodes, seed)
    t32, t64, gmm = target_pair(D, K, nodes, seed)
    g = torch.Generator().manual_seed(7400 + seed + D + K)
    eps0 = torch.randn(B, D, generator=g)
    noise_x = torch.randn(N_UPDATES, B, D, generator=g)
    noise_u = torch.rand(N_UPDATES, B, generator=g)
    with torch.no_grad():
        x = nf64.sample_eps(eps0.double())[0].float().double()                       # float32-representable
    start = oais.create_point(x, nf64.log_prob, t64.log_prob, False)
    lw_in = (oais.intermediate_log_prob(start, BETA, ALPHA, p_target) - start.log_q).detach()
    return dict(D=D, K=K, nodes=nodes, B=B, p_target=p_target, nf=nf, nf64=nf64, t32=t32, t64=t64, gmm=gmm, start=start,
                lw_in=lw_in, noise_x=noise_x, noise_u=noise_u, table=scaling_table(step), step=step)


def run_oracle(c, dtype=torch.float64, cls=TraceMetropolis, start=None, noise_x=None, noise_u=None, rows=slice(None),
               target=TARGET, tune=True, beta=BETA, table=None, i=ROW):
    """one transition of `cls` on rows `rows` of the case's (or the given) start point: (result Point, the operator)"""
    nf, tgt = (c["nf64"], c["t64"]) if dtype == torch.float64 else (c["nf"], c["t32"])
    op = cls((c["table"] if table is None else table).to(dtype), nf.log_prob, tgt.log_prob, ALPHA, c["p_target"], target, tune)
    nx = (c["noise_x"] if noise_x is None else noise_x)[:, rows].to(dtype)
    nu = (c["noise_u"] if noise_u is None else noise_u)[:, rows].to(dtype)
    out = op.transition(_point3(c["start"] if start is None else start, dtype, rows), i, beta, nx, nu)
    return out, op


def log_w_after(c, out, lw_in, beta_next=BETA_NEXT, beta=BETA):
    """ais.py:93-100 on the transition's result"""
    if beta_next == beta:
        return lw_in.clone()
    return lw_in + (oais.intermediate_log_prob(out, beta_next, ALPHA, c["p_target"]) -
                    oais.intermediate_log_prob(out, beta, ALPHA, c["p_target"]))


def mean_acceptance(trace, rows):
    """what the rule sees on the batch made of `rows` of the case (the rows of a transition do not interact)"""
    return [float(torch.mean(torch.clamp_max(t["acc"][rows], 1))) for t in trace]


@functools.lru_cache(maxsize=None)
def case(D, K, nodes, B, p_target=False):
    """Everything the tests need of one teacher-forced case, computed once and never modified."""
    c = inputs(D, K, nodes, B, p_target)
    o64, h64 = run_oracle(c, torch.float64)
    o32, h32 = run_oracle(c, torch.float32)
    tr64, tr32 = h64.traces[-1], h32.traces[-1]
    band = mc.band_of(o64)
    margins = torch.stack([t["margin"] for t in tr64])
    in_band = (margins.abs() <= band).any(0)
    acc64, acc32 = torch.stack([t["accept"] for t in tr64]), torch.stack([t["accept"] for t in tr32])
    p_accept = {B: [t["p_accept"] for t in tr64], 16: mean_acceptance(tr64, slice(0, 16))}
    return dict(c, o64=o64, o32=o32, h64=h64, h32=h32, trace=tr64, lw64=log_w_after(c, o64, c["lw_in"]),
                lw32=log_w_after(c, o32, c["lw_in"].float()), acc64=acc64, acc32=acc32, margins=margins, band=band, in_band=in_band,
                cap=int(in_band.sum()), p_accept=p_accept, table32=h32.noise_scalings.clone())


def expected_table(c, n_rows, target=TARGET):
    """the operator's table after the case's transition on its first `n_rows` rows: the statement on row ROW - 1, the rest as given"""
    t = c["table"].numpy().copy()
    t[ROW - 1] = rule_statement(t[ROW - 1], directions(c["p_accept"][n_rows], target))
    return torch.from_numpy(t)


def moved_rows(c, out, lw, factor=100.0):
    """rows of a mutant's result more than `factor` tolerances from the float64 oracle in x or in the log-weight increment"""
    inc, inc64 = lw - c["lw_in"], c["lw64"] - c["lw_in"]
    return (mc.tol_units(out.x, c["o64"].x) > factor) | (mc.tol_units(inc, inc64) > factor)


# ---- special rows -------------------------------------------------------------------------------------------------------------------
SPECIAL_ROWS = (1, 5, 11, 18)       # ratio overflows float32 only | float64 too | a NaN coordinate | log_p = -inf at the start
SPECIAL_NAMES = ("float32 overflow", "float64 overflow", "NaN coordinate", "log_p = -inf")
F32_WINDOW, F64_WINDOW = (120.0, 600.0), (710.0, 1e5)
TAIL_NOISE = 3.0


def tail_coordinate(D, which):
    """the coordinate moved into the tail: 0 for the float32 row, one beyond the first 16 lanes' first pass where D allows for
    the float64 row (ManyWell: an even one, the quartic)"""
    return 0 if which == 0 else (16 if D > 16 else 2)


@functools.lru_cache(maxsize=None)
def special(D, K, nodes, B, p_target=False):
    """A copy of the case's start with the four special rows injected (and their noise), the float32 and float64 oracle on it,
    and the same four rows alone in a batch.  The float32 oracle is the statement for these rows: float64 ACCEPTS the first."""
    c = case(D, K, nodes, B, p_target)
    nf64, t64 = c["nf64"], c["t64"]
    x = c["start"].x.clone()
    noise_x = c["noise_x"].clone()
    s = c["table"][ROW - 1].double()
    ratios = {}
    for which, (r, window) in enumerate(zip(SPECIAL_ROWS[:2], (F32_WINDOW, F64_WINDOW))):
        j = tail_coordinate(D, which)
        # the proposals step back towards the bulk by TAIL_NOISE sqrt(s_0 / s_n) scalings: log ratios within a factor sqrt(3)
        nz = -TAIL_NOISE * torch.sqrt(s[0] / s)
        noise_x[:, r, j] = nz.float()
        vs = torch.tensor(np.geomspace(1.5, 80.0, 600)).float().double()
        cand = x[r].repeat(len(vs), 1)
        cand[:, j] = vs
        base = oais.create_point(cand, nf64.log_prob, t64.log_prob, False)
        prev = oais.intermediate_log_prob(base, BETA, ALPHA, p_target)
        d = []
        for n in range(N_UPDATES):
            prop = oais.create_point(cand + noise_x[n, r].double()[None] * s[n], nf64.log_prob, t64.log_prob, False)
            d.append(oais.intermediate_log_prob(prop, BETA, ALPHA, p_target) - prev)
        d = torch.stack(d)                                                                 # [N_UPDATES, candidates]
        lo, hi = window[0] * 1.08, window[1] / 1.08
        ok = (d.min(0).values >= lo) & (d.max(0).values <= hi) & torch.isfinite(prev) & torch.isfinite(d).all(0)
        assert bool(ok.any()), f"no tail row for {SPECIAL_NAMES[which]} at D = {D}"
        k = int(ok.nonzero()[len(ok.nonzero()) // 2])
        x[r, j] = vs[k]
        ratios[r] = d[:, k]
    x[SPECIAL_ROWS[2], D - 1] = float("nan")
    start = oais.create_point(x, nf64.log_prob, t64.log_prob, False)
    start.log_p[SPECIAL_ROWS[3]] = -INF
    o64, h64 = run_oracle(c, torch.float64, start=start, noise_x=noise_x)
    o32, h32 = run_oracle(c, torch.float32, start=start, noise_x=noise_x)
    sp = list(SPECIAL_ROWS)
    alone32, ha32 = run_oracle(c, torch.float32, start=start, noise_x=noise_x, rows=sp)
    lw_in = c["lw_in"].clone()
    lw_in[sp] = (oais.intermediate_log_prob(start, BETA, ALPHA, p_target) - start.log_q)[sp]
    return dict(start=start, noise_x=noise_x, ratios=ratios, o64=o64, o32=o32, trace64=h64.traces[-1], trace32=h32.traces[-1],
                p_accept32=[t["p_accept"] for t in h32.traces[-1]], alone_p_accept32=[t["p_accept"] for t in ha32.traces[-1]],
                alone32=alone32, lw_in=lw_in)


# ---- whole calls --------------------------------------------------------------------------------------------------------------------
M_CALL, N_CALL = 3, 2
CALL_SHAPES = [(32, 3, 10, 37), (60, 2, 8, 20)]
DEAD = {37: (2, 9, 17, 20, 30, 33), 20: (0, 6, 9, 13, 17)}        # eps0 = inf there: 31 of 37 / 15 of 20 chains survive the filter
SCHEDULES = {"linear": (0.0, 0.25, 0.5, 0.75, 1.0), "repeat": (0.0, 0.3, 0.3, 0.7, 1.0)}      # repeat: beta[2] == beta[1]
# (D, K, nodes) -> (seed, largest scaling of the [M, 2] table)
CALL_PARAMS = {(32, 3, 10): (3, 0.2), (60, 2, 8): (3, 0.15)}


def call_table(step):
    """[M_CALL, N_CALL] float32, six distinct values: row j = step * 0.8^j * (1, 0.45)"""
    t = torch.tensor([[step * 0.8 ** j * f for f in (1.0, 0.45)] for j in range(M_CALL)], dtype=torch.float64).float()
    assert len(set(t.reshape(-1).tolist())) == t.numel()
    return t


@functools.lru_cache(maxsize=None)
def call_inputs(D, K, nodes, B, n_updates=N_CALL, M=M_CALL, dead=True):
    seed, step = CALL_PARAMS[(D, K, nodes)]
    nf, nf64 = flow_pair(D, K, nodes, seed)
    t32, t64, gmm = target_pair(D, K, nodes, seed)
    g = torch.Generator().manual_seed(7600 + seed + D + K + n_updates)
    eps0 = torch.randn(B, D, generator=g)
    if dead:
        eps0[list(DEAD[B])] = INF
    na = torch.randn(M, n_updates, B, D, generator=g)
    nb = torch.rand(M, n_updates, B, generator=g)
    return dict(D=D, K=K, nodes=nodes, B=B, nf=nf, nf64=nf64, t32=t32, t64=t64, gmm=gmm, eps0=eps0, na=na, nb=nb,
                table=call_table(step), p_target=False, n_alive=B - (len(DEAD[B]) if dead else 0))


def run_call(c, schedule, dtype=torch.float64, op_cls=TraceMetropolis, ais_cls=CallAIS, target=TARGET):
    nf, tgt = (c["nf64"], c["t64"]) if dtype == torch.float64 else (c["nf"], c["t32"])
    op = op_cls(c["table"].to(dtype), nf.log_prob, tgt.log_prob, ALPHA, False, target, True)
    if op_cls is MeanOverAllocatedRows:
        op.n_allocated = c["B"]
    M = c["table"].shape[0]
    ais = ais_cls(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, tgt.log_prob, op, False, ALPHA, M)
    ais.B_space = torch.tensor(schedule, dtype=torch.float64)
    assert ais.B_space.shape == (M + 2,)
    pt, lw, info = ais.sample_and_log_weights(c["eps0"].to(dtype), c["na"].to(dtype), c["nb"].to(dtype))
    return pt, lw, info, op, ais


@functools.lru_cache(maxsize=None)
def call_case(D, K, nodes, B, schedule="linear"):
    c = call_inputs(D, K, nodes, B)
    sched = SCHEDULES[schedule]
    pt64, lw64, info64, op64, ais64 = run_call(c, sched, torch.float64)
    pt32, lw32, info32, op32, _ = run_call(c, sched, torch.float32)
    nv = pt64.x.shape[0]
    in_band = torch.zeros(nv, dtype=torch.bool)
    for j, tr in enumerate(op64.traces):
        band = mc.band_of(ais64.snapshots[j + 1][0])
        for t in tr:
            in_band |= t["margin"].abs() <= band
    dec64 = torch.stack([t["accept"] for tr in op64.traces for t in tr])
    dec32 = torch.stack([t["accept"] for tr in op32.traces for t in tr])
    p_accept = np.array([[t["p_accept"] for t in tr] for tr in op64.traces])
    expected = torch.from_numpy(rule_statement(c["table"].numpy(), directions(p_accept, TARGET)))
    return dict(c, schedule=sched, pt64=pt64, lw64=lw64, info64=info64, pt32=pt32, lw32=lw32, info32=info32, dec64=dec64, dec32=dec32,
                in_band=in_band, cap=int(in_band.sum()), p_accept=p_accept, expected=expected, kept=ais64.kept,
                table32=op32.noise_scalings.clone(), snapshots=ais64.snapshots)


# ---- any number of updates ----------------------------------------------------------------------------------------------------------
NUP_SHAPE = (6, 3, 8, 17)
NUP_COUNTS = (1, 64, 65, 130)
NUP_M = 2
NUP_BIG, NUP_SMALL, NUP_ROBUST, NUP_TARGET = 2.5, 0.01, 0.15, 0.5


def nup_table(n_updates, n_dist=NUP_M):
    """[n_dist, n_updates] float32, all distinct, alternating between a scaling that rejects most proposals and one that accepts
    nearly all (the start's acceptance quantity is never refreshed, so "nearly all" wears off along 130 updates: the target of
    these cases is NUP_TARGET = 0.5).  Every mean acceptance is at least NUP_ROBUST from it, so that two of the 17 chains taking
    another decision within rounding somewhere along the way (1 / 17 = 0.06 per chain and update) cannot change a direction."""
    t = torch.tensor([[(NUP_BIG if (n + j) % 2 == 0 else NUP_SMALL) * 0.995 ** n * (1 - 0.01 * j) for n in range(n_updates)]
                      for j in range(n_dist)], dtype=torch.float64).float()
    assert len(set(t.reshape(-1).tolist())) == t.numel()
    return t


@functools.lru_cache(maxsize=None)
def nup_case(n_updates):
    """(e): one teacher-forced transition (number NUP_M, the last row) and one whole call of NUP_M transitions at NUP_SHAPE with
    `n_updates` updates each; the float64 oracle's mean acceptances and the statement of both tables."""
    D, K, nodes, B = NUP_SHAPE
    seed, _ = PARAMS[(D, K, nodes, False)]
    nf, nf64 = flow_pair(D, K, nodes, seed)
    t32, t64, _ = target_pair(D, K, nodes, seed)
    g = torch.Generator().manual_seed(7700 + n_updates)
    eps0 = torch.randn(B, D, generator=g)
    na = torch.randn(NUP_M, n_updates, B, D, generator=g)
    nb = torch.rand(NUP_M, n_updates, B, generator=g)
    table = nup_table(n_updates)
    c = dict(D=D, K=K, nodes=nodes, B=B, nf=nf, nf64=nf64, t32=t32, t64=t64, eps0=eps0, na=na, nb=nb, table=table, p_target=False)
    with torch.no_grad():
        x = nf64.sample_eps(eps0.double())[0].float().double()
    start = oais.create_point(x, nf64.log_prob, t64.log_prob, False)
    _, op = run_oracle(c, torch.float64, start=start, noise_x=na[-1], noise_u=nb[-1], i=NUP_M, target=NUP_TARGET)
    p_one = np.array([t["p_accept"] for t in op.traces[-1]])
    sched = tuple(np.linspace(0.0, 1.0, NUP_M + 2).tolist())
    pt64, lw64, _, op_call, _ = run_call(c, sched, torch.float64, target=NUP_TARGET)
    p_call = np.array([[t["p_accept"] for t in tr] for tr in op_call.traces])
    want_one = table.numpy().copy()
    want_one[NUP_M - 1] = rule_statement(want_one[NUP_M - 1], directions(p_one, NUP_TARGET))
    return dict(c, start=start, p_one=p_one, p_call=p_call, want_one=torch.from_numpy(want_one),
                want_call=torch.from_numpy(rule_statement(table.numpy(), directions(p_call, NUP_TARGET))), schedule=sched)
