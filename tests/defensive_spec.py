"""Specification of the defensive-mixture base distribution of the fused AIS call as a small CPU program - TEST
INFRASTRUCTURE, never imported by the product.  The density is the reference's
(fab/trainable_distributions/defensive_mixture.py: DefensiveMixtureDistribution with its built-in Gaussian); how the
non-finite cases, the gradient and the explicit-noise sampling are resolved is the project's own definition, and the device
follows it (include/fabhip.h: fabhip_defensive_args).

It composes oracle.flow (the flow's density and sampler) with oracle.ais (point creation, transitions, AIS driver).

Parameters: loc [D] = 0, log_scale [D] = 0, mixture_logit l (scalar) = 1.

Density, with a = log q_flow(x) + logsigmoid(l), b = log N(x; loc, exp(log_scale)) + logsigmoid(-l):
    b = sum_j(-z_j^2 / 2 - log_scale_j) - D log(2 pi) / 2 + logsigmoid(-l),   z_j = (x_j - loc_j) exp(-log_scale_j)
    m = max(a, b);  log q = m + log(exp(a - m) + exp(b - m))
    log q = -inf when m = -inf (no (-inf) - (-inf));  log q = NaN when a or b is NaN.
Gradient, closed form (never autograd through an infinite term):
    r_f = exp(a - log q)   (exactly 0 where a = -inf)
    d log q / dx_j = r_f d log q_flow / dx_j + (1 - r_f) (-(x_j - loc_j) exp(-2 log_scale_j))
    where r_f = 0 the flow's term is 0 whatever the flow's gradient holds (NaN, +-inf included).
Sampling with explicit noise eps0 [B, D] (normals) and sel [B] (uniforms in [0, 1)):
    chain i takes the flow branch iff sel_i < sigmoid(l)  (the reference's Binomial(logits=l) draw of 1):
    x = flow.sample(eps0_i), else x = loc + exp(log_scale) eps0_i;   log_q0 = log q(x) from the density direction
    (the reference's sample_and_log_prob is log_prob(sample())).
Everything downstream of log q and its gradient is oracle.ais unchanged.
"""
import math

import torch

from oracle import ais as oais


def log_prob_and_grad(nf, loc, log_scale, logit, x, with_grad=True):
    """(log q [B], d log q / dx [B, D] or None, parts) at x, in x's dtype.  parts = dict(a, b, r_f, lq_flow, g_flow)."""
    F = torch.nn.functional
    x = x.detach()
    D = x.shape[1]
    if with_grad:
        with torch.enable_grad():
            g_flow, lq_flow = oais.grad_and_value(x, nf.log_prob)
    else:
        with torch.no_grad():
            lq_flow, g_flow = nf.log_prob(x), None
    with torch.no_grad():
        logit = torch.as_tensor(logit, dtype=x.dtype)
        z = (x - loc) * torch.exp(-log_scale)
        b = torch.sum(-0.5 * (z * z) - log_scale, dim=1) - 0.5 * D * math.log(2 * math.pi) + F.logsigmoid(-logit)
        a = lq_flow + F.logsigmoid(logit)
        m = torch.maximum(a, b)                                # (propagates NaN)
        lq = m + torch.log(torch.exp(a - m) + torch.exp(b - m))
        lq = torch.where(torch.isneginf(m), m, lq)
        lq = torch.where(torch.isnan(a) | torch.isnan(b), torch.full_like(lq, float("nan")), lq)
        r_f = torch.where(torch.isneginf(a), torch.zeros_like(a), torch.exp(a - lq))
        grad = None
        if with_grad:
            g_gauss = -(x - loc) * torch.exp(-2.0 * log_scale)
            flow_term = torch.where((r_f == 0)[:, None], torch.zeros_like(g_flow), r_f[:, None] * g_flow)
            grad = flow_term + (1.0 - r_f)[:, None] * g_gauss
    return lq, grad, dict(a=a, b=b, r_f=r_f, lq_flow=lq_flow, g_flow=g_flow)


class _LogProb(torch.autograd.Function):
    """log q whose derivative w.r.t. x is the closed form: oracle.ais.create_point differentiates its log_q_fn."""

    @staticmethod
    def forward(ctx, x, mix):
        lq, grad, _ = log_prob_and_grad(mix.nf, mix.loc, mix.log_scale, mix.logit, x, with_grad=True)
        ctx.save_for_backward(grad)
        return lq

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return g[:, None] * grad, None


class DefensiveMixture:
    """The mixture over an oracle.flow flow `nf`; loc / log_scale [D] and the logit (scalar tensor) in the flow's dtype."""

    def __init__(self, nf, loc=None, log_scale=None, logit=1.0):
        dt = nf.q0.loc.dtype
        D = nf.q0.loc.shape[1]
        self.nf = nf
        self.loc = torch.zeros(D, dtype=dt) if loc is None else torch.as_tensor(loc, dtype=dt).reshape(D)
        self.log_scale = torch.zeros(D, dtype=dt) if log_scale is None else torch.as_tensor(log_scale, dtype=dt).reshape(D)
        self.logit = torch.as_tensor(logit, dtype=dt).reshape(())

    def log_prob(self, x):
        if x.requires_grad:
            return _LogProb.apply(x, self)
        return log_prob_and_grad(self.nf, self.loc, self.log_scale, self.logit, x, with_grad=False)[0]

    def log_prob_and_grad(self, x):
        return log_prob_and_grad(self.nf, self.loc, self.log_scale, self.logit, x)[:2]

    def flow_branch(self, sel):
        """sel_i < sigmoid(l), evaluated in the mixture's dtype."""
        return torch.as_tensor(sel, dtype=self.logit.dtype) < torch.sigmoid(self.logit)

    def sample_eps(self, eps0, sel):
        """(x, log_q0) for explicit noise."""
        with torch.no_grad():
            x_flow = self.nf.sample_eps(eps0)[0]
            x_gauss = self.loc + torch.exp(self.log_scale) * eps0
            x = torch.where(self.flow_branch(sel)[:, None], x_flow, x_gauss)
        return x.detach(), self.log_prob(x.detach()).detach()


def make_ais(mix: DefensiveMixture, log_p_fn, transition_operator, p_target, alpha, M, sel, cls=oais.AIS, **kw):
    """oracle.ais.AIS (or a subclass, e.g. smc_spec.SMC) over the mixture, with the branch uniforms `sel` bound in."""
    return cls(lambda e: mix.sample_eps(e, sel), mix.log_prob, log_p_fn, transition_operator, p_target, alpha, M, **kw)
