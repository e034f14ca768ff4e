"""Inputs and spec runs shared by tests/test_defensive_spec.py (CPU) and tests/test_gpu_defensive.py: the fused-call cases of
the defensive mixture, with recording transition operators so that every accept decision and its margin can be examined.
TEST INFRASTRUCTURE."""
import math

import torch

from helpers import seeded_oracle_flow
import defensive_spec as dspec
from oracle import ais as oais
from oracle import targets as otgt

D, K, NODES, B, M, L = 6, 2, 5, 40, 3, 2
STEP = 0.2
LOC, LOG_SCALE, LOGIT = 0.25, 1.0, 1.0
FAR_ROWS = (3, 17, 38)          # chains started on the Gaussian branch at radius >= 40
GAUSS_ROWS = (0, 9, 22, 31)     # further chains on the Gaussian branch, at the Gaussian's own radius

# (name, hmc, n_inner, p_target, seed): HMC L = 2 with n_outer 1 / 2 and Metropolis with 2 updates, AIS target p^2 / q and p.
# The seeds are chosen so that every accept decision of the float32 and the float64 spec run agrees and sits more than 1e-3 from
# its threshold (tests/test_defensive_spec.py: test_accept_margins_of_the_gpu_cases asserts it).
CASES = [
    ("hmc1_p2q", True, 1, False, 0),
    ("hmc2_p2q", True, 2, False, 3),
    ("hmc1_p", True, 1, True, 0),
    ("hmc2_p", True, 2, True, 1),
    ("met2_p2q", False, 2, False, 0),
    ("met2_p", False, 2, True, 0),
]


def flow(dtype=torch.float32):
    return seeded_oracle_flow(D, K, NODES, 7, std=0.05).to(dtype)


def mixture(nf):
    dt = nf.q0.loc.dtype
    return dspec.DefensiveMixture(nf, torch.full((D,), LOC, dtype=dt), torch.full((D,), LOG_SCALE, dtype=dt), LOGIT)


def inputs(hmc, n_inner, seed):
    """float32 noise: eps0 [B, D], sel [B], noise_a [M, n_inner, B, D], noise_b [M, n_inner, B]."""
    g = torch.Generator().manual_seed(1900 + seed)
    eps0 = torch.randn(B, D, generator=g)
    sel = torch.rand(B, generator=g) * 0.5                      # < sigmoid(1) = 0.731: the flow branch
    for r in GAUSS_ROWS + FAR_ROWS:
        sel[r] = 0.9
    for r in FAR_ROWS:                                          # radius = e^1 |eps0| >= 40  <=>  |eps0| >= 14.8
        eps0[r] = eps0[r] / eps0[r].norm() * 16.0
    na = torch.randn(M, n_inner, B, D, generator=g)
    nb = torch.empty(M, n_inner, B).exponential_(1.0, generator=g) if hmc else torch.rand(M, n_inner, B, generator=g)
    return eps0, sel, na, nb


class _Rec:
    """Append every value assigned to `last_margin` / `last_accept` (one per outer step / update)."""

    def _init_rec(self):
        self.__dict__["margins"], self.__dict__["accepts"] = [], []

    def __setattr__(self, k, v):
        if k == "last_margin" and v is not None:
            self.__dict__["margins"].append(v.detach().clone())
        elif k == "last_accept" and v is not None:
            self.__dict__["accepts"].append(v.detach().clone())
        object.__setattr__(self, k, v)


class RecHMC(_Rec, oais.HMC):
    def __init__(self, *a, **kw):
        self._init_rec()
        super().__init__(*a, **kw)


class RecMetropolis(_Rec, oais.Metropolis):
    """oracle.ais.Metropolis, with the acceptance ratio of every update recorded: margin = exp(delta) - u."""

    def __init__(self, *a, **kw):
        self._init_rec()
        super().__init__(*a, **kw)

    def transition(self, point, i, beta, noise_x, noise_u):
        prev = oais.intermediate_log_prob(point, beta, self.alpha, self.p_target)      # never refreshed, as in the parent
        x = point.x.clone()
        for n in range(self.n_updates):
            Bn = x.shape[0]
            prop = oais.create_point(x + noise_x[n, :Bn] * self.noise_scalings[i - 1, n], self.log_q_fn, self.log_p_fn, False)
            acc = torch.exp(oais.intermediate_log_prob(prop, beta, self.alpha, self.p_target) - prev)
            acc = torch.nan_to_num(acc, nan=0.0, posinf=0.0, neginf=0.0)
            self.last_margin = acc - noise_u[n, :Bn]
            x = torch.where((acc > noise_u[n, :Bn])[:, None], prop.x, x)
        return super().transition(point, i, beta, noise_x, noise_u)


def run_spec(case, dtype=torch.float64):
    """The spec's fused call of one case in `dtype`: dict(point, log_w, info, op, mix, x0)."""
    name, hmc, n_inner, p_target, seed = case
    nf = flow(dtype)
    mix = mixture(nf)
    tgt = otgt.ManyWell(D)
    eps0, sel, na, nb = (t.to(dtype) for t in inputs(hmc, n_inner, seed))
    alpha = None if p_target else 2.0
    if hmc:
        op = RecHMC(M, D, mix.log_prob, tgt.log_prob, alpha=alpha, p_target=p_target, epsilon=STEP, n_outer=n_inner, L=L,
                    dtype=dtype)
    else:
        op = RecMetropolis(M, D, mix.log_prob, tgt.log_prob, n_updates=n_inner, alpha=alpha, p_target=p_target,
                           max_step_size=0.2, min_step_size=0.05, dtype=dtype)
    ais = dspec.make_ais(mix, tgt.log_prob, op, p_target, alpha, M, sel)
    pt, lw, info = ais.sample_and_log_weights(eps0, na, nb, keep_snapshots=True)
    return dict(point=pt, log_w=lw, info=info, op=op, mix=mix, ais=ais, x0=ais.snapshots[0][0].x,
                base_log_w=ais.snapshots[0][0].log_p - ais.snapshots[0][0].log_q)


def radius_rows(Dn, n_rows, seed=3, dtype=torch.float64):
    """Rows at the radii 0.5, 2, 4, 40, 200 (x sqrt(Dn / 6)), cycling, on seeded directions; the last row is 1e20 (a density that is not finite)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(n_rows, Dn, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=1, keepdim=True)
    radii = torch.tensor([0.5, 2.0, 4.0, 40.0, 200.0], dtype=torch.float64) * math.sqrt(Dn / 6.0)
    x = u * radii[torch.arange(n_rows) % 5][:, None]
    x[-1] = 1e20
    return x.to(dtype)
