"""Target distributions of the hot path: ManyWell (fab/target_distributions/many_well.py:16-90,
double_well.py:31-58) and the 40-mode GMM (fab/target_distributions/gmm.py:12-66) — same constructor
arguments and `log_prob` semantics; `log_prob` runs csrc/target_device.h on the GPU.  `CoupledQuarticEnergy` / `LatticePhi4`: the
coupled-quartic family (no counterpart in the reference; tests/quartic_cases.py is its definition).  `CoupledRotorEnergy` / `LatticeXY`:
the periodic family, coupled rotors (tests/rotor_cases.py is its definition)."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _ops
from .numerical import (quadratic_function, importance_weighted_expectation,
                        effective_sample_size_over_p)


class _NativeTarget(nn.Module):
    def native_target(self):
        """The target arguments of the ops: (kind, [a, b, c, log_norm], locs or None, scales or None)."""
        raise NotImplementedError

    def _native_log_prob(self, x, with_grad=False):
        _ops.require_device(x, "x")
        lp, g = _ops.load().target_logp_grad(*self.native_target(), x.detach().contiguous().float(), bool(with_grad))
        return lp, (g if with_grad else None)

    def log_prob_and_grad(self, x):
        return self._native_log_prob(x, with_grad=True)


class _TargetLogProb(torch.autograd.Function):
    """log p(x) with d log p / dx from the same HIP launch (fabhip_target_log_prob): what generic autograd callers
    such as `grad_and_value(x, target.log_prob)` (fab/sampling_methods/base.py:50-56) and the reverse-KL baseline
    losses differentiate through."""

    @staticmethod
    def forward(ctx, target, x):
        lp, g = target._native_log_prob(x, with_grad=True)
        ctx.save_for_backward(g)
        return lp

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return None, grad_out[:, None] * g


def _target_log_prob(target, x):
    _ops.require_device(x, "x")
    if torch.is_grad_enabled() and x.requires_grad:
        return _TargetLogProb.apply(target, x)
    return target._native_log_prob(x)[0]


class ManyWellEnergy(_NativeTarget):
    """log p(x) = sum_i -(a x_{2i} + b x_{2i}^2 + c x_{2i}^4 + x_{2i+1}^2 / 2)."""

    def __init__(self, dim=4, use_gpu: bool = True, normalised: bool = False, a=-0.5, b=-6.0, c=1.0):
        super().__init__()
        assert dim % 2 == 0
        self.dim, self.n_wells = dim, dim // 2
        self._a, self._b, self._c = a, b, c
        self.normalised = normalised
        self.centre = 1.7
        self.register_buffer("_anchor", torch.zeros(1))
        if use_gpu and torch.cuda.is_available():
            self.cuda()
        self.device = "cuda" if (use_gpu and torch.cuda.is_available()) else "cpu"

    @property
    def log_Z_2D(self):
        if self._a == -0.5 and self._b == -6 and self._c == 1.0:
            return np.log(11784.50927) + 0.5 * np.log(2 * math.pi)          # double_well.py:97-101
        raise NotImplementedError

    @property
    def log_Z(self):
        return torch.tensor(self.log_Z_2D * self.n_wells)

    @property
    def Z(self):
        return torch.exp(self.log_Z)

    def native_target(self):
        log_norm = float(self.log_Z_2D * self.n_wells) if self.normalised else 0.0
        return _ops.TARGET_MANYWELL, [float(self._a), float(self._b), float(self._c), log_norm], None, None

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        return _target_log_prob(self, x)

    # ---- evaluation helpers (many_well.py:61-147, double_well.py:61-95; host-side glue, torch on the device) ----
    max_dim_for_all_modes = 40

    def _eval_device(self):
        return self._anchor.device

    def sample(self, shape) -> torch.Tensor:
        """Exact samples: per well, rejection sampling of the quartic coordinate (proposal 0.2 N(-1.7, .5) +
        0.8 N(1.7, .5), envelope 3 Z as in double_well.py:61-82) and a standard normal for the other one."""
        if not (self._a == -0.5 and self._b == -6 and self._c == 1.0):
            raise NotImplementedError
        assert len(shape) == 1
        n, dev = int(shape[0]), self._eval_device()
        need = n * self.n_wells
        mix = torch.tensor([0.2, 0.8], device=dev)
        means = torch.tensor([-1.7, 1.7], device=dev)
        log_k = math.log(11784.50927 * 3)
        got = []
        have = 0
        while have < need:
            m = int((need - have) * 3.5) + 64                      # acceptance rate is 1/3
            comp = torch.multinomial(mix, m, replacement=True)
            z = means[comp] + 0.5 * torch.randn(m, device=dev)
            log_prop = torch.logsumexp(torch.log(mix)[None, :] - 0.5 * ((z[:, None] - means[None, :]) / 0.5) ** 2
                                       - math.log(0.5 * math.sqrt(2 * math.pi)), dim=1)
            log_target = -z ** 4 + 6 * z ** 2 + 0.5 * z
            keep = torch.rand(m, device=dev).log() < log_target - log_prop - log_k
            got.append(z[keep])
            have += int(keep.sum())
        x1 = torch.cat(got)[:need].view(n, self.n_wells)
        x = torch.empty(n, self.dim, device=dev)
        x[:, 0::2] = x1
        x[:, 1::2] = torch.randn(n, self.n_wells, device=dev)
        return x

    def _well(self):
        w = self.__dict__.get("_well2d")
        if w is None:
            w = self.__dict__["_well2d"] = ManyWellEnergy(2, a=self._a, b=self._b, c=self._c)
        return w

    def log_prob_2D(self, x):
        """many_well.py:92-94: the double-well density of one coordinate pair (plotting helper), HIP like log_prob."""
        return self._well().log_prob(x)

    def energy(self, x, temperature=None):
        """double_well.py:19-23 (2-D, shape [..., 1])."""
        assert x.shape[-1] == 2, "`x` does not match `dim`"
        return -self._well().log_prob(x)[..., None] / (1.0 if temperature is None else temperature)

    def force(self, x, temperature=None):
        """double_well.py:25-28: -d energy / dx."""
        assert x.shape[-1] == 2, "`x` does not match `dim`"
        _, g = self._well().log_prob_and_grad(x.detach().contiguous().float())
        return g / (1.0 if temperature is None else temperature)

    def sample_first_dimension(self, shape):
        """double_well.py:60-82: exact samples of the quartic coordinate of one well (rejection sampling)."""
        assert len(shape) == 1
        return self._well().sample(shape)[:, 0]

    def get_modes_test_set_iterator(self, batch_size: int):
        """Points placed at the modes (x_even = +-1.7, x_odd = 0): all 2^(dim/2) of them below 40 dims, 10^4 random
        ones above (many_well.py:24-36, 68-79)."""
        dev = self._eval_device()
        if self.dim < self.max_dim_for_all_modes:
            k = torch.arange(2 ** self.n_wells, device=dev)
            bits = (k[:, None] >> torch.arange(self.n_wells - 1, -1, -1, device=dev)[None, :]) & 1
        else:
            bits = torch.randint(high=2, size=(int(1e4), self.n_wells), device=dev)
        test_set = torch.zeros(bits.shape[0], self.dim, device=dev)
        test_set[:, 0::2] = -self.centre + 2 * self.centre * bits.float()
        return list(torch.split(test_set, batch_size))

    def performance_metrics(self, samples, log_w: torch.Tensor, log_q_fn=None, batch_size=None):
        """many_well.py:96-147: accuracy of the normalisation-constant estimate over 50 splits of log_w and, given
        log_q_fn, mean flow log-prob on the mode test set / on exact samples and the forward KL estimate."""
        del samples
        n_runs = 50
        n_vals = log_w.shape[0] // n_runs
        lw = torch.stack(log_w[:n_vals * n_runs].split(n_runs), dim=-1)
        log_Z = float(self.log_Z)
        log_Z_estimate = torch.logsumexp(lw, dim=-1) - np.log(lw.shape[-1])
        info = {"relative_MSE_Z_estimate": torch.mean(torch.abs(torch.exp(log_Z_estimate - log_Z) - 1)).item(),
                "abs_MSE_log_Z_estimate": torch.mean(torch.abs(log_Z_estimate - log_Z)).item()}
        if log_q_fn is not None:
            assert batch_size is not None
            n_batches = max(lw.shape[0] // batch_size, 1)
            modes = self.get_modes_test_set_iterator(batch_size)
            with torch.no_grad():
                sum_modes = sum(float(torch.sum(log_q_fn(x))) for x in modes)
                sum_exact = sum_kl = 0.0
                for _ in range(n_batches):
                    x = self.sample((batch_size,))
                    lq = log_q_fn(x)
                    sum_exact += float(torch.sum(lq))
                    sum_kl += float(torch.sum(self.log_prob(x) - log_Z - lq))       # as written in many_well.py:137
            n_eval = batch_size * n_batches
            info.update(test_set_modes_mean_log_prob=sum_modes / sum(len(x) for x in modes),
                        test_set_exact_mean_log_prob=sum_exact / n_eval, forward_kl=sum_kl / n_eval,
                        eval_batch_size=n_eval)
        return info


class GMM(_NativeTarget):
    def __init__(self, dim, n_mixes, loc_scaling, log_var_scaling=0.1, seed=0, n_test_set_samples=1000,
                 use_gpu=True, true_expectation_estimation_n_samples=int(1e7), locs=None, scales=None):
        """`locs` / `scales` ([n_mixes, dim] each): the component means and diagonal scales per entry, in place of the
        reference's random means and one common scale (nothing is drawn then, `loc_scaling` / `log_var_scaling` are unused)."""
        super().__init__()
        self.seed, self.n_mixes, self.dim = seed, n_mixes, dim
        self.n_test_set_samples = n_test_set_samples
        self._true_expectation, self._true_expectation_n = None, int(true_expectation_estimation_n_samples)
        if locs is not None or scales is not None:
            if locs is None or scales is None or tuple(locs.shape) != (n_mixes, dim) or tuple(scales.shape) != (n_mixes, dim):
                raise ValueError(f"GMM: locs and scales must both be given as [{n_mixes}, {dim}] tensors")
            mean = locs.detach().clone().float().contiguous()
            diag = scales.detach().clone().float().contiguous()
        else:
            mean = (torch.rand((n_mixes, dim)) - 0.5) * 2 * loc_scaling      # gmm.py:22 (caller seeds torch)
            diag = F.softplus(torch.ones((n_mixes, dim)) * log_var_scaling).contiguous()
        self.register_buffer("cat_probs", torch.ones(n_mixes))
        self.register_buffer("locs", mean)
        self.register_buffer("scale_trils", torch.diag_embed(diag))
        self.register_buffer("scales", diag)
        self.device = "cuda" if (use_gpu and torch.cuda.is_available()) else "cpu"
        if self.device == "cuda":
            self.cuda()

    def native_target(self):
        return _ops.TARGET_GMM, [0.0, 0.0, 0.0, 0.0], self.locs, self.scales

    @property
    def distribution(self):
        mix = torch.distributions.Categorical(self.cat_probs)
        com = torch.distributions.MultivariateNormal(self.locs, scale_tril=self.scale_trils, validate_args=False)
        return torch.distributions.MixtureSameFamily(mix, com, validate_args=False)

    def sample(self, shape=(1,)):
        return self.distribution.sample(shape)

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        return _target_log_prob(self, x)

    # ---- evaluation helpers (gmm.py:33-36, 54-100; host-side torch, not on the hot path) ---------------------------
    expectation_function = staticmethod(quadratic_function)

    @property
    def true_expectation(self) -> torch.Tensor:
        """E_p[quadratic_function] by plain Monte Carlo; the reference estimates it in the constructor
        (gmm.py:30-33, 10^7 samples), here on first use."""
        if self._true_expectation is None:
            n, acc, done = self._true_expectation_n, 0.0, 0
            while done < n:
                m = min(n - done, 1 << 20)
                acc += float(torch.sum(self.expectation_function(self.sample((m,))).double()))
                done += m
            self._true_expectation = torch.tensor(acc / n, dtype=torch.float32)
        return self._true_expectation

    @property
    def test_set(self) -> torch.Tensor:
        return self.sample((self.n_test_set_samples,))

    def evaluate_expectation(self, samples, log_w):
        expectation = importance_weighted_expectation(self.expectation_function, samples, log_w)
        true_expectation = self.true_expectation.to(expectation.device)
        return (expectation - true_expectation) / true_expectation

    def performance_metrics(self, samples, log_w, log_q_fn=None, batch_size=None):
        bias_normed = self.evaluate_expectation(samples, log_w)
        bias_no_correction = self.evaluate_expectation(samples, torch.ones_like(log_w))
        if log_q_fn:
            with torch.no_grad():
                log_q_test = log_q_fn(self.test_set)          # two independent draws of the test set, like the
                log_p_test = self.log_prob(self.test_set)      # reference's property (gmm.py:54-56, 88-89)
            return {"test_set_mean_log_prob": torch.mean(log_q_test).item(),
                    "bias_normed": torch.abs(bias_normed).item(),
                    "bias_no_correction": torch.abs(bias_no_correction).item(),
                    "ess_over_p": effective_sample_size_over_p(log_p_test - log_q_test).item(),
                    "kl_forward": torch.mean(log_p_test - log_q_test).item()}
        return {"bias_normed": bias_normed.item(), "bias_no_correction": torch.abs(bias_no_correction).item()}


class CoupledQuarticEnergy(_NativeTarget):
    """Quartic sites with a symmetric quadratic coupling,
        log p(x) = - sum_j (a_j x_j + b_j x_j^2 + c_j x_j^4) - 1/2 x^T J x - log_norm,   D <= 64,
    evaluated by the third branch of csrc/target_device.h on every route of the fused path: lattice phi^4 (`LatticePhi4`),
    coupled double wells, soft-spin glasses, correlated Gaussians (c = 0) and ManyWell itself (J = 0).  The definition is
    tests/quartic_cases.py.  The constructor works in float64 on the host; the device holds float32 copies."""

    MAX_DIM = 64                                                    # FABHIP_MAX_DIM

    def __init__(self, site_a, site_b, site_c, coupling, normalised: bool = False, use_gpu: bool = True):
        super().__init__()
        name = type(self).__name__
        a, b, c, J = (torch.as_tensor(v).detach().to("cpu", torch.float64) for v in (site_a, site_b, site_c, coupling))
        if a.dim() != 1 or a.shape[0] < 1 or b.shape != a.shape or c.shape != a.shape or tuple(J.shape) != (a.shape[0],) * 2:
            raise ValueError(f"{name}: site_a, site_b, site_c must be [D] and coupling [D, D], got {tuple(a.shape)}, "
                             f"{tuple(b.shape)}, {tuple(c.shape)} and {tuple(J.shape)}")
        D = int(a.shape[0])
        if D > self.MAX_DIM:
            raise ValueError(f"{name}: dim = {D} is above the {self.MAX_DIM} sites the kernels hold")
        if not all(bool(torch.isfinite(v).all()) for v in (a, b, c, J)):
            raise ValueError(f"{name}: a coefficient or a coupling is not finite")
        if float((J - J.T).abs().max()) > 1e-6 * float(J.abs().max()):
            raise ValueError(f"{name}: the coupling is not symmetric (the kernels read J[k][j] for (J x)_j)")
        J = 0.5 * (J + J.T)
        if bool((c < 0).any()):
            raise ValueError(f"{name}: site_c must be >= 0 (the density could not be normalised)")
        flat = c == 0                                               # no quartic wall there: the quadratic form must hold them
        if bool(flat.any()):
            P = (2.0 * torch.diag(b) + J)[flat][:, flat]
            if float(torch.linalg.eigvalsh(P).min()) <= 0.0:
                raise ValueError(f"{name}: the density cannot be normalised: 2 diag(site_b) + coupling is not positive "
                                 "definite on the sites with site_c = 0")
        self.dim, self.normalised = D, bool(normalised)
        self._a64, self._b64, self._c64, self._J64 = a, b, c, J
        self.register_buffer("coupling", J.float().contiguous())                       # fabhip_target.locs   [D][D]
        self.register_buffer("site_coefs", torch.stack([a, b, c]).float().contiguous())    # fabhip_target.scales [3][D]
        self._log_Z = None
        if self.normalised:
            self.log_Z                                                # raises where no exact constant exists
        self.device = "cuda" if (use_gpu and torch.cuda.is_available()) else "cpu"
        if self.device == "cuda":
            self.cuda()

    # ---- the two exact cases --------------------------------------------------------------------------------------------------
    @property
    def is_gaussian(self) -> bool:
        return bool((self._c64 == 0).all())

    @property
    def is_independent(self) -> bool:
        return bool((self._J64 - torch.diag(torch.diagonal(self._J64)) == 0).all())

    def _precision(self):
        return 2.0 * torch.diag(self._b64) + self._J64

    @staticmethod
    def _site_log_z(a, b, c):
        """log of the integral of exp(-(a x + b x^2 + c x^4)) over the line (float64; trapezoid rule on a range beyond which
        the integrand is below exp(-60) of its peak - it converges geometrically for such integrands)."""
        if c == 0.0:
            return 0.5 * math.log(math.pi / b) + a * a / (4.0 * b)
        R = 1.0
        while c * R ** 4 - abs(b) * R * R - abs(a) * R < 60.0 + abs(b) ** 2 / (4.0 * c) + abs(a):
            R *= 1.25
        x = torch.linspace(-R, R, 400001, dtype=torch.float64)
        e = -(a * x + b * x * x + c * x ** 4)
        return float(torch.logsumexp(e, 0) + math.log(2.0 * R / (x.numel() - 1)))

    @property
    def log_Z(self) -> torch.Tensor:
        """float64: all c_j = 0 (Gaussian, P = 2 diag(b) + J: D/2 log 2 pi - 1/2 log det P + 1/2 a^T P^-1 a) or J diagonal
        (independent sites with the diagonal folded into b, one quadrature per site); no exact constant otherwise."""
        if self._log_Z is None:
            a, b, c = self._a64, self._b64, self._c64
            if self.is_gaussian:
                P = self._precision()
                v = 0.5 * self.dim * math.log(2.0 * math.pi) - 0.5 * torch.linalg.slogdet(P)[1] + 0.5 * a @ torch.linalg.solve(P, a)
            elif self.is_independent:
                be = b + 0.5 * torch.diagonal(self._J64)
                v = sum(self._site_log_z(float(a[j]), float(be[j]), float(c[j])) for j in range(self.dim))
            else:
                raise NotImplementedError(f"{type(self).__name__}: log_Z is known for c = 0 and for a diagonal coupling only")
            self._log_Z = torch.as_tensor(v, dtype=torch.float64)
        return self._log_Z

    @property
    def Z(self):
        return torch.exp(self.log_Z)

    def native_target(self):
        log_norm = float(self.log_Z) if self.normalised else 0.0
        return _ops.TARGET_QUARTIC, [0.0, 0.0, 0.0, log_norm], self.coupling, self.site_coefs

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        return _target_log_prob(self, x)

    def energy(self, x, temperature=None):
        assert x.shape[-1] == self.dim, "`x` does not match `dim`"
        return -self.log_prob(x)[..., None] / (1.0 if temperature is None else temperature)

    def force(self, x, temperature=None):
        assert x.shape[-1] == self.dim, "`x` does not match `dim`"
        _, g = self.log_prob_and_grad(x.detach().contiguous().float())
        return g / (1.0 if temperature is None else temperature)

    def sample(self, shape) -> torch.Tensor:
        """Exact samples of the Gaussian case: mean -P^-1 a, covariance P^-1 (Cholesky)."""
        if not self.is_gaussian:
            raise NotImplementedError(f"{type(self).__name__}: exact samples exist for c = 0 only")
        assert len(shape) == 1
        P = self._precision()
        cov = torch.linalg.inv(P)
        chol = torch.linalg.cholesky(0.5 * (cov + cov.T))
        mean = -torch.linalg.solve(P, self._a64)
        dev = self.coupling.device
        z = torch.randn(int(shape[0]), self.dim, device=dev)
        return mean.float().to(dev) + z @ chol.T.float().to(dev)


class LatticePhi4(CoupledQuarticEnergy):
    """Lattice phi^4 on a periodic lattice of prod(shape) <= 64 sites, any number of dimensions:
        S = sum_x [(1 - 2 lam) phi_x^2 + lam phi_x^4] - 2 kappa sum_x sum_mu phi_x phi_(x + mu),   log p = -S.
    a = 0, b = 1 - 2 lam, c = lam; J_xy = -2 kappa times the bonds joining x and y as the sum over (x, mu) meets them: an extent
    of 2 joins two sites twice, an extent of 1 joins a site to itself (both ends of that bond sit on the diagonal)."""

    def __init__(self, shape, kappa: float, lam: float, normalised: bool = False, use_gpu: bool = True):
        shape = tuple(int(s) for s in shape)
        if len(shape) < 1 or any(s < 1 for s in shape):
            raise ValueError(f"LatticePhi4: shape must hold positive extents, got {shape}")
        D = int(np.prod(shape))
        if D > self.MAX_DIM:
            raise ValueError(f"LatticePhi4: {shape} has {D} sites, above the {self.MAX_DIM} the kernels hold")
        idx = np.arange(D).reshape(shape)
        J = torch.zeros(D, D, dtype=torch.float64)
        for mu in range(len(shape)):
            x, y = torch.as_tensor(idx.reshape(-1)), torch.as_tensor(np.roll(idx, -1, axis=mu).reshape(-1))
            J.index_put_((x, y), torch.full((D,), -2.0 * kappa, dtype=torch.float64), accumulate=True)
            J.index_put_((y, x), torch.full((D,), -2.0 * kappa, dtype=torch.float64), accumulate=True)
        super().__init__(torch.zeros(D, dtype=torch.float64), torch.full((D,), 1.0 - 2.0 * lam, dtype=torch.float64),
                         torch.full((D,), float(lam), dtype=torch.float64), J, normalised=normalised, use_gpu=use_gpu)
        self.shape, self.kappa, self.lam = shape, float(kappa), float(lam)

    def performance_metrics(self, samples, log_w, log_q_fn=None, batch_size=None):
        """Importance-weighted <|M|>, <M^2> and the weighted share of M > 0, M the mean field of a sample: the share is the Z2
        balance (1/2 for the symmetric density; 0 or 1 when the sampler has collapsed onto one of the two modes)."""
        del log_q_fn, batch_size
        m = samples.double().mean(-1)
        w = torch.softmax(log_w.double(), 0)
        return {"abs_magnetisation": float((w * m.abs()).sum()), "magnetisation_sq": float((w * m * m).sum()),
                "positive_share": float((w * (m > 0).double()).sum())}


class CoupledRotorEnergy(_NativeTarget):
    """Coupled rotors: periodic sites with Fourier terms and couplings in angle differences, next to harmonic sites on the line,
        t_j = x_j r_j,  w_j = t_j - rint(t_j),  theta_j = 2 pi w_j,  d_jk = (w_j - w_k) - rint(w_j - w_k),
        log p(x) = sum_j [sum_{m=1..3} (A_mj cos m theta_j + B_mj sin m theta_j) - l_j x_j - q_j x_j^2]
                   + 1/2 sum_j sum_k K_jk cos(2 pi d_jk) - log_norm,                                          D <= 64,
    r_j = 1 / period_j (period_j = 0: a site on the line, r_j = 0).  The fourth branch of csrc/target_device.h evaluates it on
    every route of the fused path: lattice XY (`LatticeXY`), torsion angles with Fourier terms and harmonic bonds, a torus shared
    with `CircularCoupledRQSFlow` (`for_flow`).  The definition is tests/rotor_cases.py.  The kernels read the coupling as a
    neighbour table that lists every bond from both ends; this class builds it from the symmetric matrix, so the contract is
    kept here.  Checks run in float64 on the host; the device holds float32 copies."""

    MAX_DIM = 64                                                    # FABHIP_MAX_DIM
    N_HARMONICS = 3

    def __init__(self, period, fourier_cos, fourier_sin, coupling, line_linear=None, line_quadratic=None,
                 normalised: bool = False, use_gpu: bool = True):
        super().__init__()
        name = type(self).__name__
        h = lambda v: torch.as_tensor(v).detach().to("cpu", torch.float64)             # noqa: E731
        P = h(period)
        if P.dim() != 1 or P.shape[0] < 1:
            raise ValueError(f"{name}: period must be [D] with D >= 1, got {tuple(P.shape)}")
        D = int(P.shape[0])
        if D > self.MAX_DIM:
            raise ValueError(f"{name}: dim = {D} is above the {self.MAX_DIM} sites the kernels hold")
        A, B, K = h(fourier_cos), h(fourier_sin), h(coupling)
        l = torch.zeros(D, dtype=torch.float64) if line_linear is None else h(line_linear)
        q = torch.zeros(D, dtype=torch.float64) if line_quadratic is None else h(line_quadratic)
        A, B = (v[None] if v.dim() == 1 else v for v in (A, B))                        # [D]: the first harmonic alone
        if A.dim() != 2 or A.shape[1] != D or not 1 <= A.shape[0] <= self.N_HARMONICS or B.shape != A.shape \
                or tuple(K.shape) != (D, D) or l.shape != (D,) or q.shape != (D,):
            raise ValueError(f"{name}: fourier_cos and fourier_sin must be [D] or [m, D] with m <= {self.N_HARMONICS}, coupling "
                             f"[D, D], line_linear and line_quadratic [D] for D = {D}, got {tuple(A.shape)}, {tuple(B.shape)}, "
                             f"{tuple(K.shape)}, {tuple(l.shape)} and {tuple(q.shape)}")
        pad = torch.zeros(self.N_HARMONICS - A.shape[0], D, dtype=torch.float64)
        A, B = torch.cat([A, pad]), torch.cat([B, pad])
        if not all(bool(torch.isfinite(v).all()) for v in (P, A, B, K, l, q)):
            raise ValueError(f"{name}: a period, a coefficient or a coupling is not finite")
        if bool((P < 0).any()):
            raise ValueError(f"{name}: a period is negative (0 marks a site on the line)")
        if float((K - K.T).abs().max()) > 1e-6 * float(K.abs().max()):
            raise ValueError(f"{name}: the coupling is not symmetric (every bond is listed from both ends)")
        K = 0.5 * (K + K.T)
        if bool((torch.diagonal(K) != 0).any()):
            raise ValueError(f"{name}: the coupling has a non-zero diagonal (a site's bond to itself is a constant)")
        line = P == 0
        if bool((K[line] != 0).any()):
            raise ValueError(f"{name}: the coupling touches a site on the line (it acts on angle differences)")
        if bool(((l != 0) | (q != 0))[~line].any()):
            raise ValueError(f"{name}: line_linear / line_quadratic are set on a periodic site (the density would not be periodic)")
        if bool(((A != 0) | (B != 0)).any(0)[line].any()):
            raise ValueError(f"{name}: Fourier coefficients are set on a site on the line (it has no angle)")
        if bool((q[line] <= 0).any()):
            raise ValueError(f"{name}: line_quadratic must be > 0 on a site on the line (the density could not be normalised)")
        self.dim, self.normalised = D, bool(normalised)
        rate = torch.where(line, torch.zeros_like(P), 1.0 / torch.where(line, torch.ones_like(P), P))
        self._P64, self._A64, self._B64, self._K64, self._l64, self._q64, self._line = P, A, B, K, l, q, line
        idx, kap = self.neighbour_table(K)
        self.n_neighbours = int(idx.shape[0])
        self.register_buffer("table", torch.cat([idx, kap]).float().contiguous())                  # fabhip_target.locs   [2 NB][D]
        self.register_buffer("site_rows", torch.cat([A, B, rate[None], l[None], q[None]]).float().contiguous())    # .scales [9][D]
        self.register_buffer("period", P.float())
        self._log_Z = None
        if self.normalised:
            self.log_Z                                                # raises where no exact constant exists
        self.device = "cuda" if (use_gpu and torch.cuda.is_available()) else "cpu"
        if self.device == "cuda":
            self.cuda()

    @staticmethod
    def neighbour_table(K):
        """(indices [NB, D], couplings [NB, D]) in float64: column j lists the k with K[j, k] != 0 in ascending k and pads with
        k = j, kap = 0; NB = max(1, largest count)."""
        D = K.shape[0]
        rows = [torch.nonzero(K[j] != 0).flatten() for j in range(D)]
        NB = max(1, max(int(r.numel()) for r in rows))
        idx = torch.arange(D, dtype=torch.float64)[None].repeat(NB, 1)
        kap = torch.zeros(NB, D, dtype=torch.float64)
        for j, r in enumerate(rows):
            idx[:r.numel(), j] = r.double()
            kap[:r.numel(), j] = K[j, r]
        return idx, kap

    @classmethod
    def for_flow(cls, spline_flow, fourier_cos, fourier_sin, coupling, line_linear=None, line_quadratic=None, **kw):
        """The target on the torus of `spline_flow` (a CircularCoupledRQSFlow): period_j = 2 tail_bound_j on the flow's circular
        coordinates, 0 elsewhere."""
        circ, tb = spline_flow._circ.cpu(), spline_flow._tail_bound.detach().cpu().double()
        return cls(torch.where(circ, 2.0 * tb, torch.zeros_like(tb)), fourier_cos, fourier_sin, coupling, line_linear,
                   line_quadratic, **kw)

    # ---- the exact cases ------------------------------------------------------------------------------------------------------
    @property
    def is_independent(self) -> bool:
        return bool((self._K64 == 0).all())

    @property
    def is_single_harmonic(self) -> bool:
        return bool((self._A64[1:] == 0).all() and (self._B64[1:] == 0).all())

    def _site_log_z(self, j):
        """log of the integral of site j's factor over one period (periodic) or over the line, float64"""
        if bool(self._line[j]):
            l, q = float(self._l64[j]), float(self._q64[j])
            return 0.5 * math.log(math.pi / q) + l * l / (4.0 * q)
        P, A, B = float(self._P64[j]), self._A64[:, j], self._B64[:, j]
        if bool((A[1:] == 0).all() and (B[1:] == 0).all()):
            kappa = torch.sqrt(A[0] * A[0] + B[0] * B[0])
            return math.log(P) + float(torch.log(torch.special.i0e(kappa)) + kappa)
        n = 4096                                                     # periodic and analytic: the trapezoid rule converges spectrally
        th = 2.0 * math.pi * torch.arange(n, dtype=torch.float64) / n
        m = torch.arange(1, self.N_HARMONICS + 1, dtype=torch.float64)[:, None]
        e = (A[:, None] * torch.cos(m * th) + B[:, None] * torch.sin(m * th)).sum(0)
        return float(torch.logsumexp(e, 0)) + math.log(P / n)

    @property
    def log_Z(self) -> torch.Tensor:
        """float64, over one period of every periodic site and the line of every other; known without a coupling only."""
        if self._log_Z is None:
            if not self.is_independent:
                raise NotImplementedError(f"{type(self).__name__}: log_Z is known without a coupling only")
            self._log_Z = torch.as_tensor(sum(self._site_log_z(j) for j in range(self.dim)), dtype=torch.float64)
        return self._log_Z

    @property
    def Z(self):
        return torch.exp(self.log_Z)

    def native_target(self):
        log_norm = float(self.log_Z) if self.normalised else 0.0
        return _ops.TARGET_ROTOR, [0.0, 0.0, 0.0, log_norm], self.table, self.site_rows

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        return _target_log_prob(self, x)

    def energy(self, x, temperature=None):
        assert x.shape[-1] == self.dim, "`x` does not match `dim`"
        return -self.log_prob(x)[..., None] / (1.0 if temperature is None else temperature)

    def force(self, x, temperature=None):
        assert x.shape[-1] == self.dim, "`x` does not match `dim`"
        _, g = self.log_prob_and_grad(x.detach().contiguous().float())
        return g / (1.0 if temperature is None else temperature)

    def wrap(self, x: torch.Tensor) -> torch.Tensor:
        """Periodic coordinates mapped to [-P/2, P/2); coordinates on the line and coordinates already inside are returned as
        they are (so that wrap is idempotent)."""
        P = self.period.to(x.device, x.dtype)
        safe = torch.where(P > 0, P, torch.ones_like(P))
        y = x - safe * torch.floor(x / safe + 0.5)
        y = torch.where(y >= 0.5 * safe, y - safe, torch.where(y < -0.5 * safe, y + safe, y))
        inside = (x >= -0.5 * safe) & (x < 0.5 * safe)
        return torch.where((P > 0) & ~inside, y, x)

    def sample(self, shape) -> torch.Tensor:
        """Exact samples without a coupling and with single-harmonic sites: von Mises angles (drawn on the host) and Gaussians."""
        if not (self.is_independent and self.is_single_harmonic):
            raise NotImplementedError(f"{type(self).__name__}: exact samples exist without a coupling and for single-harmonic "
                                      "sites only")
        assert len(shape) == 1
        n = int(shape[0])
        A, B, P, line = self._A64[0], self._B64[0], self._P64, self._line
        kappa, phi = torch.sqrt(A * A + B * B), torch.atan2(B, A)
        x = torch.empty(n, self.dim, dtype=torch.float64)
        for j in range(self.dim):
            if bool(line[j]):
                l, q = float(self._l64[j]), float(self._q64[j])
                x[:, j] = -l / (2.0 * q) + torch.randn(n, dtype=torch.float64) / math.sqrt(2.0 * q)
            elif float(kappa[j]) < 1e-12:
                x[:, j] = (torch.rand(n, dtype=torch.float64) - 0.5) * P[j]
            else:
                th = torch.distributions.VonMises(phi[j], kappa[j]).sample((n,))
                x[:, j] = th * P[j] / (2.0 * math.pi)
        return x.float().to(self.table.device)


class LatticeXY(CoupledRotorEnergy):
    """The XY model on a periodic lattice of prod(shape) <= 64 sites, any number of dimensions:
        log p = coupling sum over bonds cos(theta_x - theta_y) + field sum_x cos(theta_x),   theta_x = 2 pi x / period.
    The bonds are those the sum over (x, mu) meets: an extent of 2 joins two sites twice (K = 2 coupling between them), an extent
    of 1 joins a site to itself - a constant, left out of the table."""

    def __init__(self, shape, coupling: float, field: float = 0.0, period: float = 2.0 * math.pi, normalised: bool = False,
                 use_gpu: bool = True):
        shape = tuple(int(s) for s in shape)
        if len(shape) < 1 or any(s < 1 for s in shape):
            raise ValueError(f"LatticeXY: shape must hold positive extents, got {shape}")
        D = int(np.prod(shape))
        if D > self.MAX_DIM:
            raise ValueError(f"LatticeXY: {shape} has {D} sites, above the {self.MAX_DIM} the kernels hold")
        idx = np.arange(D).reshape(shape)
        K = torch.zeros(D, D, dtype=torch.float64)
        n_bonds = 0
        for mu in range(len(shape)):
            if shape[mu] == 1:
                continue
            x, y = torch.as_tensor(idx.reshape(-1)), torch.as_tensor(np.roll(idx, -1, axis=mu).reshape(-1))
            K.index_put_((x, y), torch.full((D,), float(coupling), dtype=torch.float64), accumulate=True)
            K.index_put_((y, x), torch.full((D,), float(coupling), dtype=torch.float64), accumulate=True)
            n_bonds += D
        super().__init__(torch.full((D,), float(period), dtype=torch.float64), torch.full((D,), float(field), dtype=torch.float64),
                         torch.zeros(D, dtype=torch.float64), K, normalised=normalised, use_gpu=use_gpu)
        self.shape, self.coupling_strength, self.field, self.n_bonds = shape, float(coupling), float(field), n_bonds

    def performance_metrics(self, samples, log_w, log_q_fn=None, batch_size=None):
        """Importance-weighted |mean_x exp(i theta_x)| (the magnetisation per site), its square, and the mean cosine over the
        nearest-neighbour bonds (1 for an ordered lattice, 0 without bonds or without order)."""
        del log_q_fn, batch_size
        th = samples.double().cpu() * (2.0 * math.pi / float(self._P64[0]))
        w = torch.softmax(log_w.double().cpu(), 0)
        m2 = torch.cos(th).mean(-1) ** 2 + torch.sin(th).mean(-1) ** 2
        f = th.reshape((th.shape[0],) + self.shape)
        nn_cos = torch.zeros(th.shape[0], dtype=torch.float64)
        for mu in range(len(self.shape)):
            if self.shape[mu] > 1:
                nn_cos += torch.cos(f - torch.roll(f, -1, dims=mu + 1)).reshape(th.shape[0], -1).sum(-1)
        nn_cos = nn_cos / max(self.n_bonds, 1)
        return {"abs_magnetisation": float((w * m2.sqrt()).sum()), "magnetisation_sq": float((w * m2).sum()),
                "neighbour_cosine": float((w * nn_cos).sum())}
