"""Specification of the adaptive annealing schedule (distribution_spacing_type="adaptive": ESS-decay bisection) as a small CPU
program - TEST INFRASTRUCTURE, never imported by the product.  The reference knows two fixed schedules only; like the SMC mode's,
this definition is the project's own, and the device follows it (include/fabhip.h: fabhip_next_beta).

It composes oracle.ais (point creation, transitions, intermediate_log_prob), oracle.numerical (fixed_point_weights) and
tests/smc_spec.py (the resampling step).  With M transitions, decay rho in (0, 1) and pi_beta = intermediate_log_prob:

1. The chain initialisation runs with beta_1 := 0: log_w = pi_0 - log q0; the "chain init" filter as ever.  betas = [0].
2. beta_1 = next_beta(log_w, log_q, log_p, 0); log_w += pi_{beta_1} - pi_0.
3. For j = 1 .. M: [resample_threshold set: the resampling step of smc_spec, noise_r[j - 1];] transition j at beta_j with index
   j (epsilons[j - 1] and the step-size rule as ever); beta_{j+1} = next_beta at the new point (after transition M:
   beta_{M+1} = 1 without a decision); beta_{j+1} != beta_j: log_w += pi_{beta_{j+1}} - pi_{beta_j}.
4. Once beta has reached 1 the remaining transitions run at beta = 1: no decision (it could only answer 1), no increment.
5. "chain end" filter, ESS, log Z as ever.

next_beta over the n0 live rows, stated so that a device reproduces it bit for bit:

    lw = float32 log_w;  d = float32(log_p - log_q)  (one float32 subtract);  s = float64(1 if p_target else alpha)
    ess_of(v): W = fixed_point_weights(v); S1i = sum W, S2i = sum W^2 (exact integers); S1i == 0 -> 0.0, else the three-operation
               float64 expression of smc_spec.decide, step 2, with n0
    cand(delta) = float32(lw + float32((float64(delta) * s) * float64(d)))
    ess0 = ess_of(lw);  thr = float64(rho) * ess0;  room = 1.0 - float64(beta)
    not room > 0: 1.0                                   (1 evaluation)
    ess_of(cand(room)) >= thr: 1.0                      (2 evaluations)
    lo, hi = 0.0, room;  K times: mid = 0.5 * (lo + hi);  ess_of(cand(mid)) >= thr ? lo = mid : hi = mid
    delta = lo if lo > 0 else hi                        (the floor room / 2^K: every step moves)
    min(float64(beta) + delta, 1.0)

The criterion is relative (keep rho of the ESS the weights have now), so it reads the same after a resampling step has made the
weights equal.  Non-finite rows weigh 0.  ESS need not be monotone in delta: the bisection is the definition, whatever it finds.
Besides beta_next the function reports ess0, the ESS at the chosen step (of the floor step - below thr - where the floor was
taken; of the last candidate evaluated where there was no bisection), the number of evaluations and whether the floor was taken.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import ais as oais
from oracle.numerical import effective_sample_size, fixed_point_weights
import smc_spec


class NextBeta(NamedTuple):
    beta_next: float
    ess0: float
    ess_choice: float
    evaluations: int
    floor: bool

    def as_out4(self):
        """The four doubles the device writes."""
        return [self.beta_next, self.ess0, self.ess_choice, float(self.evaluations + 65536 * int(self.floor))]


def ess_of(v) -> np.float64:
    v = np.asarray(v, dtype=np.float32)
    n0 = v.shape[0]
    W = fixed_point_weights(v)
    S1i = sum(int(w) for w in W)
    if S1i == 0:
        return np.float64(0.0)
    S2i = sum(int(w) * int(w) for w in W)
    hi, lo = divmod(S2i, 1 << 64)
    S1 = np.float64(np.uint64(S1i))
    S2 = np.float64(hi) * np.float64(2.0 ** 64) + np.float64(np.uint64(lo))
    return (S1 * S1) / (np.float64(n0) * S2)


def next_beta(log_w, log_q, log_p, beta, alpha, p_target: bool, rho, K: int = 24) -> NextBeta:
    lw = np.asarray(log_w, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(log_p, dtype=np.float32) - np.asarray(log_q, dtype=np.float32)).astype(np.float32)
    s = np.float64(1.0 if p_target else alpha)

    def cand(delta):
        with np.errstate(invalid="ignore", over="ignore"):
            t = ((np.float64(delta) * s) * d.astype(np.float64)).astype(np.float32)
            return (lw + t).astype(np.float32)

    beta = np.float64(beta)
    ess0 = ess_of(lw)
    thr = np.float64(rho) * ess0
    room = np.float64(1.0) - beta
    if not room > 0:
        return NextBeta(1.0, float(ess0), float(ess0), 1, False)
    e = ess_of(cand(room))
    if e >= thr:
        return NextBeta(1.0, float(ess0), float(e), 2, False)
    lo, hi, ess_lo, ess_hi = np.float64(0.0), room, ess0, e
    for _ in range(K):
        mid = np.float64(0.5) * (lo + hi)
        e = ess_of(cand(mid))
        if e >= thr:
            lo, ess_lo = mid, e
        else:
            hi, ess_hi = mid, e
    floor = not lo > 0
    delta, at = (hi, ess_hi) if floor else (lo, ess_lo)
    return NextBeta(float(min(beta + delta, np.float64(1.0))), float(ess0), float(at), 2 + K, bool(floor))


class Decision(NamedTuple):
    step: int                 # made after transition `step` (0: after the chain initialisation)
    beta: float
    result: NextBeta


class Adaptive(smc_spec.SMC):
    """oracle.ais.AIS / smc_spec.SMC on an adaptive schedule.  `force_betas` [M + 2]: the run uses this schedule (the decisions
    are still taken and recorded).  `teacher_log_w_pre` [M] arrays: the resampling step of transition j decides on these weights
    instead of the run's own (GPU tests: the device's), as tests/test_gpu_smc.py teacher-forces its decisions."""

    def __init__(self, *args, ess_decay: float = 0.7, **kwargs):
        super().__init__(*args, **kwargs)
        assert 0.0 < ess_decay < 1.0
        self.ess_decay = ess_decay
        self.betas: Optional[list] = None
        self.decisions: Optional[list] = None
        self.log_w_after: Optional[list] = None      # log_w after the increment of step j (index 0: after step 2)

    def _pi(self, point, beta):
        return oais.intermediate_log_prob(point, torch.tensor(float(beta), dtype=torch.float64), self.alpha, self.p_target)

    def sample_and_log_weights(self, eps0, noise_a, noise_b, noise_r=None, force_betas=None, teacher_log_w_pre=None):
        tau = self.resample_threshold
        assert tau is None or (noise_r is not None and len(noise_r) == self.M), "one uniform per transition"
        forced = None if force_betas is None else [float(b) for b in force_betas]
        assert forced is None or (len(forced) == self.M + 2 and forced[0] == 0.0 and forced[-1] == 1.0)
        batch_size = eps0.shape[0]
        x, log_q0 = self.sample_eps_fn(eps0)
        point = oais.create_point(x, self.log_q_fn, self.log_p_fn, with_grad=self.transition_operator.uses_grad_info,
                                  log_q_x=log_q0)
        log_w = (self._pi(point, 0.0) - log_q0).detach()
        point, log_w = oais.remove_nan_and_infs(point, log_w, "chain init")
        with torch.no_grad():
            ess_base = effective_sample_size(point.log_p - point.log_q).item()
        decisions = []

        def choose(step, beta):
            r = next_beta(log_w.numpy(), point.log_q.detach().numpy(), point.log_p.detach().numpy(), beta, self.alpha,
                          self.p_target, self.ess_decay)
            decisions.append(Decision(step, float(beta), r))
            return r.beta_next

        b1 = choose(0, 0.0)
        betas = [0.0, forced[1] if forced is not None else b1]
        if betas[1] != 0.0:
            log_w = log_w + (self._pi(point, betas[1]) - self._pi(point, 0.0))
        after = [log_w.clone()]
        trace = smc_spec.SMCTrace([], [], [], [], [])
        for j in range(1, self.M + 1):
            bj = betas[j]
            if tau is not None:
                trace.log_w_pre.append(log_w.clone())
                seen = log_w if teacher_log_w_pre is None else torch.as_tensor(np.asarray(teacher_log_w_pre[j - 1], np.float32))
                d = smc_spec.decide(seen.numpy(), tau, float(noise_r[j - 1]))
                if d.resampled:
                    point, log_w = smc_spec.gather_point(point, d.ancestors), torch.full_like(log_w, d.log_w_common)
                trace.resampled.append(d.resampled); trace.ess.append(d.ess); trace.ancestors.append(d.ancestors)
                trace.log_w_post.append(log_w.clone())
            point = self.transition_operator.transition(point, j, torch.tensor(bj, dtype=torch.float64), noise_a[j - 1],
                                                        noise_b[j - 1])
            nxt = 1.0
            if j < self.M:
                nxt = choose(j, bj) if bj < 1.0 else 1.0
                if forced is not None:
                    nxt = forced[j + 1]
            if nxt != bj:
                log_w = log_w + (self._pi(point, nxt) - self._pi(point, bj))
            betas.append(nxt)
            after.append(log_w.clone())
        point, log_w = oais.remove_nan_and_infs(point, log_w, "chain end")
        with torch.no_grad():
            ess_ais = effective_sample_size(log_w).item()
            lz = torch.logsumexp(log_w, dim=0)
            log_Z = (lz - torch.log(torch.ones_like(lz) * batch_size)).item()
        self.betas, self.decisions, self.log_w_after = betas, decisions, after
        self.trace = trace if tau is not None else None
        return point, log_w.detach(), oais.LoggingInfo(ess_base, ess_ais, log_Z)
