"""DefensiveMixtureDistribution with the reference's interface (fab/trainable_distributions/defensive_mixture.py:9-71):
a base distribution whose density is bounded from below by a Gaussian,

    log q(x) = logsumexp(log q_flow(x) + logsigmoid(l), log N(x; loc, exp(log_scale)) + logsigmoid(-l)),

so that the AIS target p^2 / q stays bounded where the flow's float32 density underflows (defensive importance sampling).
Parameters under the reference's names, shapes and initial values: `loc [D]` = 0, `log_scale [D]` = 0, `mixture_logit` = 1.

With a fab_torch_amd RealNVP inside, an AIS call over the mixture is ONE fused op (torch.ops.fabhip.ais_run_ext ->
fabhip_ais_run_ext: the 16-chain kernels' *_mix instantiations read the three parameter tensors directly); operators stepped
from Python evaluate density + gradient with one launch (`log_prob_and_grad` -> fabhip::defensive_log_prob).  `log_prob` is
differentiable w.r.t. the flow's and the three mixture parameters: composed in torch on top of the flow's differentiable
`log_prob`.  Sampling is not differentiable, as in the reference.  Definition of the semantics: tests/defensive_spec.py."""
import math
from typing import Tuple

import torch
from torch import nn

from . import _ops
from .flow import RealNVP


def mixture_log_prob(log_q_flow: torch.Tensor, x: torch.Tensor, loc: torch.Tensor, log_scale: torch.Tensor,
                     logit: torch.Tensor) -> torch.Tensor:
    """The mixture density from the flow's, differentiable in every argument.  A flow term of -inf (float32 underflow far
    out) is masked out of the logsumexp instead of differentiated through: its responsibility is exactly 0."""
    F = torch.nn.functional
    z = (x - loc) * torch.exp(-log_scale)
    b = torch.sum(-0.5 * z * z - log_scale, dim=-1) - 0.5 * x.shape[-1] * math.log(2 * math.pi) + F.logsigmoid(-logit)
    a = log_q_flow + F.logsigmoid(logit)
    dead = torch.isneginf(a)
    a_safe = torch.where(dead, b.detach(), a)                 # (finite stand-in: no gradient flows to the masked branch)
    both = torch.logsumexp(torch.stack((a_safe, b), dim=0), dim=0)
    return torch.where(dead, b, both)


class DefensiveMixtureDistribution(nn.Module):
    def __init__(self, flow, defensive_dist=None):
        super().__init__()
        if defensive_dist is not None:
            raise NotImplementedError("DefensiveMixtureDistribution: a user-supplied defensive_dist is not supported; the "
                                      "built-in diagonal Gaussian (loc, log_scale; defensive_dist=None) is the supported case")
        assert len(flow.event_shape) == 1
        self.flow = flow
        self.dim = int(flow.event_shape[0])
        ref = next(flow.parameters())
        self.loc = nn.Parameter(torch.zeros(self.dim, dtype=torch.float32, device=ref.device))
        self.log_scale = nn.Parameter(torch.zeros(self.dim, dtype=torch.float32, device=ref.device))
        self.mixture_logit = nn.Parameter(torch.tensor(1.0, dtype=torch.float32, device=ref.device))

    @property
    def event_shape(self) -> Tuple[int, ...]:
        return (self.dim,)

    @property
    def precision(self):
        return getattr(self.flow, "precision", None)

    @property
    def is_native(self) -> bool:
        """The fused call applies: a RealNVP inside (a spline flow goes down the generic path)."""
        return isinstance(self.flow, RealNVP)

    def native(self, need_inverse: bool = True):
        """The flow arguments of the ops (the RealNVP's packed image); the mixture's own parameters travel as tensors."""
        return self.flow.native(need_inverse)

    def mix_args(self) -> tuple:
        """(loc, log_scale, mixture_logit [1]) as the ops take them: the parameter tensors themselves, no copy."""
        if not self.is_native:
            raise _ops.FabhipError("DefensiveMixtureDistribution: the fused path needs a fab_torch_amd RealNVP inside")
        for t in (self.loc, self.log_scale, self.mixture_logit):
            _ops.require_device(t, "DefensiveMixtureDistribution parameters")
        return self.loc.detach(), self.log_scale.detach(), self.mixture_logit.detach().reshape(1)

    def _refuse_fast(self):
        if self.is_native and (_ops.precision_of(self.flow) == _ops.PRECISION_FAST or
                               (_ops.precision_of(self.flow) == _ops.PRECISION_DEFAULT and int(_ops.load().get_fast_mode()))):
            raise _ops.FabhipError('DefensiveMixtureDistribution runs in fp32 only: precision = "fast" (bf16 fast mode) is not '
                                   'available for the mixture kernels; set flow.precision = "fp32"')

    # ---- Distribution interface (fab/types_.py:8-27) ----------------------------------------------------------------------
    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        params_need_grad = any(p.requires_grad for p in self.parameters())
        if self.is_native and not (torch.is_grad_enabled() and (x.requires_grad or params_need_grad)):
            return self.log_prob_and_grad(x, with_grad=False)[0]
        # Rows where the flow's density has underflowed to -inf carry non-finite intermediates on the flow's tape, and a zero
        # coefficient times those is NaN in the parameter-gradient GEMMs.  They are read off the differentiable pass's OWN output
        # (one small host read, next to the trainers' finite-loss checks); only when there are any, the pass is run again with
        # `loc` in their place (the first graph is dropped; the other rows keep their bits, rows being independent) and their
        # flow term is masked to -inf again.
        lq_flow = self.flow.log_prob(x)
        dead = torch.isneginf(lq_flow.detach())
        if bool(dead.any()):
            x_flow = torch.where(dead[:, None], self.loc.detach().to(x.dtype), x)
            lq_flow = self.flow.log_prob(x_flow)
            lq_flow = torch.where(dead, torch.full_like(lq_flow, -math.inf), lq_flow)
        return mixture_log_prob(lq_flow, x, self.loc, self.log_scale, self.mixture_logit)

    def log_prob_and_grad(self, x: torch.Tensor, with_grad: bool = True):
        """(log q(x), d log q / dx) in one launch - what `grad_and_value(x, mixture.log_prob)` computes, with the closed-form
        gradient (finite where the flow's density has underflowed)."""
        if not self.is_native:
            xg = x.detach().requires_grad_(True)
            with torch.enable_grad():
                y = mixture_log_prob(self.flow.log_prob(xg), xg, self.loc.detach(), self.log_scale.detach(),
                                     self.mixture_logit.detach())
                g = torch.autograd.grad(y, xg, grad_outputs=torch.ones_like(y))[0] if with_grad else None
            return y.detach(), g
        _ops.require_device(x, "x")
        self._refuse_fast()
        lq, g = _ops.load().defensive_log_prob(*self.flow.native(need_inverse=False), *self.mix_args(),
                                               x.detach().contiguous().float(), bool(with_grad), _ops.precision_of(self.flow))
        return lq, (g if with_grad else None)

    @torch.no_grad()
    def sample(self, shape: Tuple, eps: torch.Tensor = None, sel: torch.Tensor = None) -> torch.Tensor:
        """Not differentiable (defensive_mixture.py:56-65).  Row i takes the flow's sample iff sel_i < sigmoid(mixture_logit) -
        the reference's Binomial(logits=l) draw of 1 - and loc + exp(log_scale) eps_i otherwise (one eps per row serves both
        branches, as in the fused call)."""
        assert len(shape) == 1
        n, dev = int(shape[0]), self.loc.device
        if eps is None:
            eps = torch.randn((n, self.dim), dtype=torch.float32, device=dev)
        if sel is None:
            sel = torch.rand(n, dtype=torch.float32, device=dev)
        if isinstance(self.flow, RealNVP):
            x_flow = self.flow.native_sample(eps)[0]
        else:
            x_flow = self.flow.sample(shape)
        x_gauss = self.loc + torch.exp(self.log_scale) * eps
        return torch.where((sel < torch.sigmoid(self.mixture_logit))[:, None], x_flow, x_gauss)

    @torch.no_grad()
    def sample_and_log_prob(self, shape: Tuple, eps: torch.Tensor = None, sel: torch.Tensor = None):
        """log_prob(sample()), without gradient, as in the reference (defensive_mixture.py:67-71)."""
        x = self.sample(shape, eps=eps, sel=sel)
        return x, self.log_prob(x)
