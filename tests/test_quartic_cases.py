"""The coupled-quartic target's definition (quartic_cases.QuarticStatement) and the conditions test_gpu_quartic.py relies on,
asserted on the CPU from the statement and the oracle alone: the written-out gradient is float64 autograd; J = 0 with ManyWell's
coefficients is oracle.targets.ManyWell; c = 0 is a multivariate normal up to log_Z; the independent-site log_Z is ManyWell's
constant; LatticePhi4's coupling is the lattice action; the float32 statement stays inside `helpers.close` of the float64 one on
every direct case (also with the rows moved by 16 ulps); every one-line mutant moves a compared value beyond the tolerance on
those rows; no accept decision of a transition case sits inside the rounding band; the constructor refuses what it must."""
import math

import numpy as np
import pytest
import torch

import hmc_mass_cases as mc
import quartic_cases as qc
import target_cases as tc
from helpers import close, worst
from oracle import targets as otgt

M = qc.M_CHAIN


def _autograd(fn, x):
    x = x.clone().requires_grad_(True)
    lp = fn(x)
    return lp.detach(), torch.autograd.grad(lp, x, torch.ones_like(lp))[0]


def _targets():
    import fab_torch_amd as fa
    return fa


# ---- the statement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", qc.DIMS)
def test_written_out_gradient_is_float64_autograd(D):
    c = qc.case(D)
    x = c["rows"]["wide"]
    lp, g = c["st64"].log_prob_and_grad(x)
    lp_a, g_a = _autograd(lambda v: c["st64"].log_prob_and_grad(v)[0], x)
    assert torch.equal(lp, lp_a) and close(g, g_a, 1e-12, atol=1e-10), worst(g, g_a, 1e-12)
    # ... against the formula written once more with a matrix product (the statement's loop over k is the same sum)
    a, b, cc, J = (v.double() for v in (c["a"], c["b"], c["c"], c["J"]))
    plain = -(a * x + b * x ** 2 + cc * x ** 4).sum(-1) - 0.5 * torch.einsum("bi,ij,bj->b", x, J, x) - qc.LOG_NORM
    assert close(lp, plain, 1e-12, atol=1e-9)
    # the autograd node of the statement hands out the written-out gradient
    assert torch.equal(_autograd(c["st64"].log_prob, x)[1], g)
    lp_s, g_s = c["st64"].log_prob_and_grad(c["rows"]["special"])
    assert torch.isnan(lp_s[0]) and not torch.isfinite(lp_s[1]) and float(lp_s[2]) == -qc.LOG_NORM
    assert bool(torch.isfinite(g_s[2]).all()) and torch.equal(g_s[2], -a)


@pytest.mark.parametrize("D", tc.MW_DIMS)
def test_without_coupling_and_with_manywell_coefficients_it_is_the_oracle_manywell(D):
    a, b, c, J = qc.manywell_form(D)
    st = qc.QuarticStatement(a, b, c, J)
    for name in ("wide", "modes"):
        x = tc.manywell_rows(D)[name]
        lp, g = st.log_prob_and_grad(x)
        lp_o, g_o = _autograd(otgt.ManyWell(D).log_prob, x)
        assert close(lp, lp_o, 1e-12, atol=1e-9) and close(g, g_o, 1e-12, atol=1e-9), name


@pytest.mark.parametrize("D", [1, 2, 5, 17])
def test_without_quartic_terms_it_is_a_multivariate_normal_and_log_Z_is_its_constant(D):
    fa = _targets()
    g = torch.Generator().manual_seed(70 + D)
    a = torch.empty(D, dtype=torch.float64).uniform_(-0.5, 0.5, generator=g)
    R = torch.randn(D, D, generator=g, dtype=torch.float64)
    P = R @ R.T / D + 0.5 * torch.eye(D, dtype=torch.float64)              # positive definite, dense
    b = torch.empty(D, dtype=torch.float64).uniform_(0.1, 0.4, generator=g)
    J = P - 2.0 * torch.diag(b)
    t = fa.CoupledQuarticEnergy(a, b, torch.zeros(D), J, use_gpu=False)
    st = qc.QuarticStatement(a, b, torch.zeros(D, dtype=torch.float64), 0.5 * (J + J.T))
    x = torch.randn(32, D, generator=g, dtype=torch.float64) * 1.5
    cov = torch.linalg.inv(P)
    mvn = torch.distributions.MultivariateNormal(-cov @ a, covariance_matrix=0.5 * (cov + cov.T))
    assert t.log_Z.dtype == torch.float64
    assert close(st.log_prob(x) - t.log_Z, mvn.log_prob(x), 1e-10, atol=1e-9)
    assert fa.CoupledQuarticEnergy(a, b, torch.zeros(D), J, normalised=True, use_gpu=False).native_target()[1][3] == float(t.log_Z)
    s = t.sample((20000,)).double()
    assert s.shape == (20000, D) and float((s.mean(0) + cov @ a).abs().max()) < 0.05 * float(cov.diagonal().max().sqrt()) + 0.02


@pytest.mark.parametrize("D", [2, 6, 64])
def test_independent_site_log_Z_is_the_manywell_constant(D):
    fa = _targets()
    a, b, c, J = qc.manywell_form(D)
    t = fa.CoupledQuarticEnergy(a, b, c, J, use_gpu=False)
    # double_well.py:97-101 gives the constant with ten digits
    assert abs(float(t.log_Z) - otgt.ManyWell(D).log_Z) < 2e-9 * otgt.ManyWell(D).log_Z * 10
    # a diagonal coupling is folded into b: the same density written the other way round has the same constant
    t2 = fa.CoupledQuarticEnergy(a, b - 0.25, c, 0.5 * torch.eye(D, dtype=torch.float64), use_gpu=False)
    assert abs(float(t2.log_Z) - float(t.log_Z)) < 1e-9 * abs(float(t.log_Z))
    with pytest.raises(NotImplementedError):
        J2 = J.clone()
        J2[0, 1] = J2[1, 0] = 0.1
        fa.CoupledQuarticEnergy(a, b, c.clamp(min=0.1), J2, use_gpu=False).log_Z


# ---- the lattice ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", qc.LATTICES)
def test_lattice_phi4_coupling_is_the_lattice_action(shape):
    fa = _targets()
    kappa, lam = 0.3, 0.02 + 0.1 * len(shape)
    t = fa.LatticePhi4(shape, kappa, lam, use_gpu=False)
    D = int(np.prod(shape))
    assert t.dim == D and t.coupling.shape == (D, D) and t.site_coefs.shape == (3, D)
    J = t._J64
    assert torch.equal(J, J.T)
    # every site has 2 ndim bonds, counted with multiplicity (extent 2: a double bond; extent 1: both ends on the diagonal)
    bonds = torch.round(J / (-2.0 * kappa))
    assert float((J + 2.0 * kappa * bonds).abs().max()) < 1e-15 and bool((bonds >= 0).all())
    assert torch.equal(bonds.sum(1), torch.full((D,), 2.0 * len(shape), dtype=torch.float64))
    assert torch.equal(t._a64, torch.zeros(D, dtype=torch.float64)) and float(t._b64[0]) == 1 - 2 * lam and float(t._c64[0]) == lam
    st = qc.QuarticStatement(t._a64, t._b64, t._c64, J)
    g = torch.Generator().manual_seed(11)
    phi = torch.randn(7, D, generator=g, dtype=torch.float64)
    S = qc.lattice_action(shape, kappa, lam, phi)
    assert close(-st.log_prob(phi), S, 1e-12, atol=1e-10)
    assert close(st.log_prob(-phi), st.log_prob(phi), 1e-12, atol=1e-10)                         # Z2
    for mu in range(len(shape)):                                                                 # lattice translations
        moved = torch.roll(phi.reshape((7,) + tuple(shape)), 1, dims=mu + 1).reshape(7, D)
        assert close(st.log_prob(moved), st.log_prob(phi), 1e-12, atol=1e-10)


def test_lattice_phi4_metrics_read_the_z2_balance():
    fa = _targets()
    t = fa.LatticePhi4((4, 4), 0.3, 0.02, use_gpu=False)
    x = torch.cat([torch.full((3, 16), 1.0), torch.full((1, 16), -2.0)])
    m = t.performance_metrics(x, torch.log(torch.tensor([1.0, 1.0, 1.0, 3.0], dtype=torch.float64)))
    assert abs(m["positive_share"] - 0.5) < 1e-12 and abs(m["abs_magnetisation"] - 1.5) < 1e-12 and abs(m["magnetisation_sq"] - 2.5) < 1e-12
    with pytest.raises(ValueError, match="sites"):
        fa.LatticePhi4((9, 8), 0.3, 0.02, use_gpu=False)


# ---- the direct cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", qc.DIMS)
def test_float32_statement_stays_inside_the_tolerance_also_under_sixteen_ulp_nudges(D):
    c = qc.case(D)
    assert torch.equal(c["J"], c["J"].T) and bool((c["J"] != 0).all()) and len(set(torch.cat([c["a"], c["b"], c["c"]]).tolist())) == 3 * D
    g = torch.Generator().manual_seed(5 + D)
    rows = [c["rows"]["wide"]] + [qc.nudged(c["rows"]["wide"], g) for _ in range(4)]
    for x in rows:
        assert float(x.abs().max()) <= 3.0 + 1e-4
        lp64, g64 = c["st64"].log_prob_and_grad(x)
        lp32, g32 = c["st32"].log_prob_and_grad(x.float())
        assert lp32.dtype == torch.float32
        print(f"MEASURE D={D} | fp32 statement | log p {worst(lp32, lp64):.3f} | grad {worst(g32, g64):.3f}")
        assert worst(lp32, lp64) < 0.25 and worst(g32, g64) < 0.25
    lp64, g64 = c["ref"]["special"]
    lp32, g32 = c["st32"].log_prob_and_grad(c["rows"]["special"].float())
    assert close(lp32, lp64) and close(g32, g64)             # (`close` asks for equal non-finite patterns)


@pytest.mark.parametrize("D,name", [(D, n) for D in qc.DIMS for n, m in qc.MUTANTS.items() if m[2](D)])
def test_every_one_line_mutant_moves_a_compared_value_beyond_the_tolerance(D, name):
    cls, where, _ = qc.MUTANTS[name]               # (listed only where the mutant is not the statement itself: D = 1, D = 16, ...)
    c = qc.case(D)
    x = c["rows"]["wide"]
    m = cls(c["a"], c["b"], c["c"], c["J"], log_norm=c["log_norm"])
    lp, g = m.log_prob_and_grad(x)
    lp64, g64 = c["ref"]["wide"]
    u_lp, u_g = mc.tol_units(lp[:, None], lp64[:, None]), mc.tol_units(g, g64)
    print(f"MEASURE D={D} {name} | rows beyond the tolerance: log p {int((u_lp > 1).sum())}, grad {int((u_g > 1).sum())} of {x.shape[0]}")
    if where in ("both", "log_p"):
        assert float(u_lp.max()) > 100 and int((u_lp > 10).sum()) >= x.shape[0] // 4
    if where in ("both", "grad"):
        assert float(u_g.max()) > 100 and int((u_g > 10).sum()) >= x.shape[0] // 4
    if where == "log_p":
        assert torch.equal(g, g64)
    if where == "grad":
        assert torch.equal(lp, lp64)


# ---- the transition cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", qc.T_SHAPES + qc.EXTRA_SHAPES, ids=str)
def test_no_accept_decision_of_a_transition_case_sits_inside_the_rounding_band(shape):
    c = qc.t_case(*shape)
    assert c["cap"] == 0 and torch.equal(c["cls32"], c["cls64"])
    acc = [float(a.float().mean()) for a in c["accept"]]
    assert all(0.15 < a < 0.98 for a in acc) and any(a < 0.95 for a in acc), acc
    o32, o64 = c["o32"], c["o64"]
    for k in ("x", "log_q", "log_p", "grad_log_p"):
        assert worst(getattr(o32, k), getattr(o64, k)) < 0.5, k
    assert worst(c["lw32"], c["lw64"]) < 0.5
    assert float(qc.perturbed_worst(*shape).max()) < 0.5
    # the target matters to the case: without the coupling's gradient the chains end elsewhere
    out, _, start = qc.run_oracle(*shape, target_cls=qc.CouplingGradientWithHalf)
    assert int(qc.moved_chains(out, start, c).sum()) >= shape[3] // 4


def test_metropolis_case_conditions():
    c = qc.metropolis_case()
    assert c["cap"] == 0 and torch.equal(c["acc64"], c["acc32"])
    assert all(0.15 < float(a) < 0.9 for a in c["acc64"].float().mean(1))
    assert worst(c["o32"].x, c["o64"].x) < 0.5 and worst(c["lw32"], c["lw64"]) < 0.5


@pytest.mark.parametrize("shape,mix", [(s, False) for s in qc.CHAIN_SHAPES] + [(qc.MIX_SHAPE, True)], ids=str)
def test_whole_call_case_conditions(shape, mix):
    c = qc.chain_case(*shape, mix=mix)
    assert c["cap"] == 0 and torch.equal(c["dec32"], c["dec64"])
    assert 0.1 < float(c["dec64"].float().mean()) < 0.98
    p32, p64 = c["pt32"], c["pt64"]
    for k in ("x", "log_q", "log_p"):
        assert worst(getattr(p32, k), getattr(p64, k), M * 1e-4) < 0.5, k
    assert worst(c["lw32"], c["lw64"], M * 1e-4) < 0.5 and worst(p32.grad_log_q, p64.grad_log_q, M * 5e-4) < 0.5


# ---- the constructor -----------------------------------------------------------------------------------------------------------------
def test_constructor_refuses_by_name():
    fa = _targets()
    D = 4
    a, b, c, J = torch.zeros(D), torch.full((D,), -1.0), torch.full((D,), 0.5), torch.zeros(D, D)
    ok = fa.CoupledQuarticEnergy(a, b, c, J, use_gpu=False)
    assert ok.dim == D and ok.coupling.dtype == torch.float32 and ok.site_coefs.shape == (3, D)
    bad = [("above the 64", (torch.zeros(65), torch.ones(65), torch.ones(65), torch.zeros(65, 65))),
           ("must be", (a, b[:3], c, J)), ("must be", (a, b, c, torch.zeros(D, D + 1))), ("must be", (a, b, c, torch.zeros(D * D))),
           ("must be", (torch.zeros(0), torch.zeros(0), torch.zeros(0), torch.zeros(0, 0))),
           ("not finite", (a, b, torch.tensor([0.5, float("nan"), 0.5, 0.5]), J)),
           ("not finite", (a, b, c, torch.full((D, D), float("inf")))),
           ("not symmetric", (a, b, c, torch.triu(torch.ones(D, D), 1))),
           ("site_c must be >= 0", (a, b, torch.tensor([0.5, -0.1, 0.5, 0.5]), J)),
           ("cannot be normalised", (a, b, torch.tensor([0.5, 0.0, 0.5, 0.5]), J)),                 # b < 0 where c = 0
           ("cannot be normalised", (a, torch.full((D,), 0.1), torch.zeros(D), -torch.ones(D, D)))]  # 0.2 I - 1 1^T is indefinite
    for match, args in bad:
        with pytest.raises(ValueError, match=match):
            fa.CoupledQuarticEnergy(*args, use_gpu=False)
    # symmetric to 1e-6 of the largest entry is taken, and stored as (J + J^T) / 2
    Jn = torch.zeros(D, D, dtype=torch.float64)
    Jn[0, 1], Jn[1, 0] = 1.0, 1.0 + 5e-7
    t = fa.CoupledQuarticEnergy(a, b, c, Jn, use_gpu=False)
    assert float(t._J64[0, 1]) == float(t._J64[1, 0]) == 1.0 + 2.5e-7
    with pytest.raises(NotImplementedError):
        fa.CoupledQuarticEnergy(a, b, c, Jn, normalised=True, use_gpu=False)
    with pytest.raises(NotImplementedError):
        ok.sample((3,))
