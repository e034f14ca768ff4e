"""Specification of the SMC mode of the fused AIS call (adaptive systematic resampling in front of every transition) as a
small CPU program - TEST INFRASTRUCTURE, never imported by the product.  The reference has no such mode: like the systematic
resampler's, this definition is the project's own, and the device follows it (include/fabhip.h: fabhip_smc_args).

It composes oracle.ais (point creation, transitions, intermediate_log_prob) with oracle.numerical (fixed_point_weights,
systematic_fixed).  Before transition j = 1 .. M, with n0 chains alive after the "chain init" filter, threshold tau and one
uniform u_j in [0, 1):

1. W = fixed_point_weights(log_w[:n0])  (uint64; rows with a NaN / infinite log_w weigh 0).
2. The arithmetic of the decision, stated so that a device reproduces it bit for bit:
       S1i = sum W            exact integer (< 2^62)
       S2i = sum W^2          exact integer (< 2^98); hi, lo = divmod(S2i, 2^64)
       S1  = float64(S1i)                                   (round to nearest even)
       S2  = float64(hi) * 2^64 + float64(lo)               (hi < 2^34 is exact, lo rounds to nearest even, one rounded add)
       ess = (S1 * S1) / (float64(n0) * S2)                 (three individually rounded float64 operations, in this order)
   S1i == 0: ess is reported as 0 and nothing is resampled.
3. ess < tau: anc = systematic_fixed(log_w[:n0], u_j, n0); x, log q, log p and (HMC) both gradients are gathered with anc, and
   every log_w becomes  float32(float64(m) + log(S1 * 2^-36 / float64(n0)))  with m the largest finite log_w (float32):
   the log of the mean weight, so logsumexp(log_w) - the tail's log Z estimator - is what it was, up to the 2^-36 quantum.
4. Otherwise the step is the identity.
5. Transition j and its log-weight increment run as in oracle.ais.AIS.  Nothing is resampled after the last transition.

tau = None is oracle.ais.AIS itself, tau > 1 resamples before every transition, tau <= 0 never does.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import ais as oais
from oracle.numerical import FIX_BITS, effective_sample_size, fixed_point_weights, systematic_fixed


class Decision(NamedTuple):
    resampled: bool
    ess: float                # float64 value of step 2
    ancestors: np.ndarray     # int64 [n0]; the identity where nothing is resampled
    log_w_common: float       # float32 value every log_w takes when resampled (nan otherwise)


def decide(log_w, tau: float, u: float) -> Decision:
    """Steps 1 - 3 for the n0 = len(log_w) live chains."""
    lw = np.asarray(log_w, dtype=np.float32)
    n0 = lw.shape[0]
    W = fixed_point_weights(lw)
    S1i = sum(int(w) for w in W)
    S2i = sum(int(w) * int(w) for w in W)
    ident = np.arange(n0, dtype=np.int64)
    if S1i == 0:
        return Decision(False, 0.0, ident, float("nan"))
    hi, lo = divmod(S2i, 1 << 64)
    S1 = np.float64(np.uint64(S1i))
    S2 = np.float64(hi) * np.float64(2.0 ** 64) + np.float64(np.uint64(lo))
    ess = (S1 * S1) / (np.float64(n0) * S2)
    if not ess < np.float64(tau):
        return Decision(False, float(ess), ident, float("nan"))
    assert 0.0 <= float(u) < 1.0
    anc = systematic_fixed(lw, float(u), n0)
    m = lw[np.isfinite(lw)].max()
    common = np.float32(np.float64(m) + np.log(S1 * np.float64(2.0 ** -FIX_BITS) / np.float64(n0)))
    return Decision(True, float(ess), anc, float(common))


def gather_point(point: oais.Point, anc) -> oais.Point:
    idx = torch.as_tensor(np.asarray(anc), dtype=torch.long)
    g = lambda t: None if t is None else t[idx].clone()      # noqa: E731
    return oais.Point(g(point.x), g(point.log_q), g(point.log_p), g(point.grad_log_q), g(point.grad_log_p))


def resample_step(point: oais.Point, log_w: torch.Tensor, tau: float, u: float):
    """(point, log_w, Decision) after the resampling step in front of a transition."""
    d = decide(log_w.detach().numpy(), tau, u)
    if not d.resampled:
        return point, log_w, d
    return gather_point(point, d.ancestors), torch.full_like(log_w, d.log_w_common), d


class SMCTrace(NamedTuple):
    resampled: list           # [M] bool
    ess: list                 # [M] float
    ancestors: list           # [M] int64 arrays [n0]
    log_w_pre: list           # [M] float32 tensors [n0]: the weights each decision saw
    log_w_post: list          # [M] float32 tensors [n0]: the weights transition j started from


class SMC(oais.AIS):
    """oracle.ais.AIS with the resampling step; `resample_threshold=None` runs the parent's method unchanged."""

    def __init__(self, *args, resample_threshold: Optional[float] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.resample_threshold = resample_threshold
        self.trace: Optional[SMCTrace] = None

    def sample_and_log_weights(self, eps0, noise_a, noise_b, noise_r=None, keep_snapshots=False):
        tau = self.resample_threshold
        if tau is None:
            return super().sample_and_log_weights(eps0, noise_a, noise_b, keep_snapshots=keep_snapshots)
        assert noise_r is not None and len(noise_r) == self.M, "one uniform per transition"
        batch_size = eps0.shape[0]
        x, log_q0 = self.sample_eps_fn(eps0)
        point = oais.create_point(x, self.log_q_fn, self.log_p_fn,
                                  with_grad=self.transition_operator.uses_grad_info, log_q_x=log_q0)
        log_w = (oais.intermediate_log_prob(point, self.B_space[1], self.alpha, self.p_target) - log_q0).detach()
        point, log_w = oais.remove_nan_and_infs(point, log_w, "chain init")
        with torch.no_grad():
            ess_base = effective_sample_size(point.log_p - point.log_q).item()
        trace = SMCTrace([], [], [], [], [])
        snaps = [(point.clone(), log_w.clone())] if keep_snapshots else None
        for j in range(1, self.M + 1):
            trace.log_w_pre.append(log_w.clone())
            point, log_w, d = resample_step(point, log_w, tau, float(noise_r[j - 1]))
            trace.resampled.append(d.resampled); trace.ess.append(d.ess); trace.ancestors.append(d.ancestors)
            trace.log_w_post.append(log_w.clone())
            point = self.transition_operator.transition(point, j, self.B_space[j], noise_a[j - 1], noise_b[j - 1])
            if self.B_space[j + 1] != self.B_space[j]:
                num = oais.intermediate_log_prob(point, self.B_space[j + 1], self.alpha, self.p_target)
                den = oais.intermediate_log_prob(point, self.B_space[j], self.alpha, self.p_target)
                log_w = log_w + (num - den)
            if keep_snapshots:
                snaps.append((point.clone(), log_w.clone()))
        point, log_w = oais.remove_nan_and_infs(point, log_w, "chain end")
        with torch.no_grad():
            ess_ais = effective_sample_size(log_w).item()
            lz = torch.logsumexp(log_w, dim=0)
            log_Z = (lz - torch.log(torch.ones_like(lz) * batch_size)).item()
        self.snapshots, self.trace = snaps, trace
        return point, log_w.detach(), oais.LoggingInfo(ess_base, ess_ais, log_Z)
