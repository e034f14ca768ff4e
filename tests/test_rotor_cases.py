"""The coupled-rotor target's definition (rotor_cases.RotorStatement) and the conditions test_gpu_rotor.py relies on, asserted on
the CPU from the statement and the oracle alone: the written-out gradient is float64 autograd and the statement is the definition
written with torch's own sine and cosine; without a coupling and with one harmonic it is a product of von Mises densities; on
line-only sites it is the quartic statement; LatticeXY's table is the lattice action; log_Z by quadrature is the closed form; the
float32 statement stays inside a quarter of `helpers.close` of the float64 one on every direct case (also with the rows moved by
16 ulps) and has its non-finite pattern; every one-line mutant moves a compared value beyond the tolerance on those rows; no accept
decision of a transition case sits inside the rounding band; the constructor refuses what it must."""
import math

import numpy as np
import pytest
import torch

import hmc_mass_cases as mc
import quartic_cases as qc
import rotor_cases as rc
from helpers import close, worst

M = rc.M_CHAIN


@pytest.fixture(autouse=True)
def one_thread():
    """The fp32 oracle's sums follow the thread count; the GPU tests run it on one thread (tests/conftest.py), so this file does."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _autograd(fn, x):
    x = x.clone().requires_grad_(True)
    lp = fn(x)
    return lp.detach(), torch.autograd.grad(lp, x, torch.ones_like(lp))[0]


def _targets():
    import fab_torch_amd as fa
    return fa


def _native_form(c):
    """constructor arguments of the package's class for a case"""
    return dict(period=c["P"], fourier_cos=c["A"], fourier_sin=c["B"], coupling=c["K"], line_linear=c["l"], line_quadratic=c["q"])


# ---- the statement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,density", rc.all_cases())
def test_written_out_gradient_is_float64_autograd_and_the_statement_is_the_plain_formula(D, density):
    c = rc.case(D, density)
    x = c["rows_x"]["wide"]
    lp, g = c["st64"].log_prob_and_grad(x)
    lp_a, g_a = _autograd(lambda v: c["st64"].log_prob_and_grad(v)[0], x)
    assert torch.equal(lp, lp_a) and close(g, g_a, 1e-11, atol=1e-9), worst(g, g_a, 1e-11)
    # ... against the definition's first line with torch's cos / sin of 2 pi x r and the coupling as a matrix, and ITS autograd
    lp_p, g_p = _autograd(lambda v: rc.plain_log_prob(c["rows"], c["K32"], v, rc.LOG_NORM), x)
    assert close(lp, lp_p, 1e-11, atol=1e-9) and close(g, g_p, 1e-10, atol=1e-8), (worst(lp, lp_p, 1e-11), worst(g, g_p, 1e-10))
    # the autograd node of the statement hands out the written-out gradient
    assert torch.equal(_autograd(c["st64"].log_prob, x)[1], g)
    # the table: every bond from both ends, ascending k, padded with k = j and kap = 0, NB = max(1, largest count)
    NB, T = c["NB"], c["table"].double()
    counts = (c["K32"] != 0).sum(1)
    assert NB == max(1, int(counts.max())) <= 63 and T.shape == (2 * NB, D)
    for j in range(D):
        ks = T[:NB, j].long().tolist()
        n = int(counts[j])
        assert ks[:n] == sorted(ks[:n]) == torch.nonzero(c["K32"][j]).flatten().tolist() and all(k == j for k in ks[n:])
        assert torch.equal(T[NB:NB + n, j], c["K32"][j, ks[:n]].double()) and bool((T[NB + n:, j] == 0).all())
    if D > 2:
        assert c["has_line"] and 0 < int((c["P"] > 0).sum()) < D
    if (D, density) == (64, "dense"):
        assert NB >= 40
    # the special rows: NaN from a NaN, from +inf on a periodic site (inf - inf) and from +inf on a line site (0 inf); zeros
    lp_s, g_s = c["st64"].log_prob_and_grad(c["rows_x"]["special"])
    assert torch.isnan(lp_s[0]) and torch.isnan(lp_s[1]) and torch.isnan(lp_s[2]) == c["has_line"]
    zero = c["rows"][0:3].double().sum() + 0.5 * c["K32"].double().sum() - rc.LOG_NORM         # cos 0 = 1 everywhere
    assert abs(float(lp_s[3]) - float(zero)) < 1e-9 and bool(torch.isfinite(g_s[3]).all())
    # a NaN site spoils its own gradient and its neighbours', not the others'
    j = D // 2
    touched = torch.zeros(D, dtype=torch.bool)
    touched[j] = True
    touched |= c["K32"][j] != 0
    assert torch.equal(torch.isnan(g_s[0]), touched)


@pytest.mark.parametrize("D", [1, 2, 7, 33])
def test_without_coupling_and_with_one_harmonic_it_is_a_von_mises_product(D):
    fa = _targets()
    g = torch.Generator().manual_seed(80 + D)
    P = torch.empty(D, dtype=torch.float64).uniform_(2.0, 7.0, generator=g)
    A, B = (torch.empty(D, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g) for _ in range(2))
    t = fa.CoupledRotorEnergy(P, A, B, torch.zeros(D, D), use_gpu=False)
    assert t.log_Z.dtype == torch.float64 and t.n_neighbours == 1 and t.table.shape == (2, D)
    st = rc.RotorStatement(t.site_rows, t.table)
    x = (torch.rand(32, D, generator=g, dtype=torch.float64) - 0.5) * 3 * P
    vm = torch.distributions.VonMises(torch.atan2(B, A), torch.sqrt(A * A + B * B))
    # density in x: the von Mises density in theta times d theta / dx = 2 pi / P
    want = (vm.log_prob(2 * math.pi * x / P) + torch.log(2 * math.pi / P)).sum(-1)
    assert close(st.log_prob(x) - t.log_Z, want, 1e-6, atol=1e-6), worst(st.log_prob(x) - t.log_Z, want, 1e-6)   # (float32 rows)
    tn = fa.CoupledRotorEnergy(P, A, B, torch.zeros(D, D), normalised=True, use_gpu=False)
    assert tn.native_target()[1][3] == float(t.log_Z) and tn.native_target()[0] == 4
    torch.manual_seed(3)
    s = t.sample((20000,)).double()
    th = 2 * math.pi * s / P
    assert s.shape == (20000, D) and bool((s.abs() <= 0.5 * P + 1e-5).all())
    R = torch.special.i1(vm.concentration) / torch.special.i0(vm.concentration)            # E exp(i (theta - mu)) of a von Mises
    assert float((torch.cos(th - vm.loc).mean(0) - R).abs().max()) < 0.03 and float(torch.sin(th - vm.loc).mean(0).abs().max()) < 0.03


@pytest.mark.parametrize("D", [1, 5, 17, 64])
def test_on_line_only_sites_it_is_the_quartic_statement(D):
    g = torch.Generator().manual_seed(90 + D)
    l = torch.empty(D, dtype=torch.float64).uniform_(-0.5, 0.5, generator=g)
    q = torch.empty(D, dtype=torch.float64).uniform_(0.2, 1.5, generator=g)
    z = torch.zeros(D, dtype=torch.float64)
    rows, table, _ = rc.pack(z, torch.zeros(3, D, dtype=torch.float64), torch.zeros(3, D, dtype=torch.float64), l, q,
                             torch.zeros(D, D, dtype=torch.float64))
    x = torch.randn(32, D, generator=g, dtype=torch.float64) * 2
    for dtype in (torch.float64, torch.float32):
        lp, gr = rc.RotorStatement(rows, table, dtype, 0.5).log_prob_and_grad(x)
        lq, gq = qc.QuarticStatement(rows[7], rows[8], z.float(), torch.zeros(D, D), dtype, 0.5).log_prob_and_grad(x)
        assert torch.equal(lp, lq) and torch.equal(gr, gq)
    fa = _targets()
    t = fa.CoupledRotorEnergy(z, z, z, torch.zeros(D, D), l, q, use_gpu=False)
    tq = fa.CoupledQuarticEnergy(l, q, z, torch.zeros(D, D), use_gpu=False)
    assert abs(float(t.log_Z) - float(tq.log_Z)) < 1e-12 * max(1.0, abs(float(tq.log_Z)))
    torch.manual_seed(4)
    s = t.sample((20000,)).double()
    assert float((s.mean(0) + l / (2 * q)).abs().max()) < 0.05 and float((s.var(0) * 2 * q - 1).abs().max()) < 0.08


@pytest.mark.parametrize("harmonics", [1, 2, 3])
def test_log_Z_by_quadrature_is_the_closed_form(harmonics):
    """one harmonic: log(P I0(|A1 + i B1|)) is used, and the trapezoid branch (reached through a vanishing second harmonic) agrees
    with it to rounding; every count of harmonics: against a brute-force sum over 200 000 points of the period"""
    fa = _targets()
    D = 3
    g = torch.Generator().manual_seed(60 + harmonics)
    P = torch.tensor([2.0, 5.5, 0.0], dtype=torch.float64)
    A = torch.empty(3, D, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    B = torch.empty(3, D, dtype=torch.float64).uniform_(-1.0, 1.0, generator=g)
    A[harmonics:], B[harmonics:] = 0.0, 0.0
    A[:, 2], B[:, 2] = 0.0, 0.0
    l, q = torch.tensor([0.0, 0.0, 0.3], dtype=torch.float64), torch.tensor([0.0, 0.0, 0.7], dtype=torch.float64)
    t = fa.CoupledRotorEnergy(P, A, B, torch.zeros(D, D), l, q, use_gpu=False)
    want = 0.5 * math.log(math.pi / 0.7) + 0.09 / 2.8
    for j in range(2):
        x = torch.linspace(0.0, float(P[j]), 200001, dtype=torch.float64)[:-1]
        th = 2 * math.pi * x / P[j]
        e = sum(A[m, j] * torch.cos((m + 1) * th) + B[m, j] * torch.sin((m + 1) * th) for m in range(3))
        want += float(torch.logsumexp(e, 0)) + math.log(float(P[j]) / 200000)
    assert abs(float(t.log_Z) - want) < 1e-10 * max(1.0, abs(want)), (float(t.log_Z), want)
    if harmonics == 1:
        closed = sum(math.log(float(P[j]) * float(torch.special.i0(torch.sqrt(A[0, j] ** 2 + B[0, j] ** 2)))) for j in range(2))
        assert abs(float(t.log_Z) - (closed + 0.5 * math.log(math.pi / 0.7) + 0.09 / 2.8)) < 1e-12 * max(1.0, abs(want))
        A2 = A.clone()
        A2[1, 0] = 1e-300                                                        # the trapezoid branch on site 0
        t2 = fa.CoupledRotorEnergy(P, A2, B, torch.zeros(D, D), l, q, use_gpu=False)
        assert not t2.is_single_harmonic and abs(float(t2.log_Z) - float(t.log_Z)) < 1e-12 * max(1.0, abs(want))
    Kc = torch.zeros(D, D, dtype=torch.float64)
    Kc[0, 1] = Kc[1, 0] = 0.2
    with pytest.raises(NotImplementedError, match="coupling"):
        fa.CoupledRotorEnergy(P, A, B, Kc, l, q, use_gpu=False).log_Z
    with pytest.raises(NotImplementedError, match="coupling"):
        fa.CoupledRotorEnergy(P, A, B, Kc, l, q, normalised=True, use_gpu=False)
    with pytest.raises(NotImplementedError):
        fa.CoupledRotorEnergy(P, A, B, Kc, l, q, use_gpu=False).sample((3,))
    if harmonics > 1:
        with pytest.raises(NotImplementedError):
            t.sample((3,))


# ---- the lattice ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rc.LATTICES)
def test_lattice_xy_table_is_the_lattice_action(shape):
    fa = _targets()
    J, field, period = 0.7, 0.3, 2 * math.pi if len(shape) != 2 else 3.0
    t = fa.LatticeXY(shape, J, field, period, use_gpu=False)
    D = int(np.prod(shape))
    active = [s for s in shape if s > 1]
    NB = max(1, sum(1 if s == 2 else 2 for s in active))                      # an extent of 2: ONE neighbour with a double bond
    assert t.dim == D and t.table.shape == (2 * NB, D) and t.site_rows.shape == (9, D) and t.n_bonds == D * len(active)
    K = t._K64
    assert torch.equal(K, K.T) and bool((torch.diagonal(K) == 0).all())
    assert torch.equal(K.sum(1), torch.full((D,), 2.0 * J * len(active), dtype=torch.float64))
    st = rc.RotorStatement(t.site_rows, t.table)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(7, D, generator=g, dtype=torch.float64) * period
    S = rc.lattice_action(shape, J, field, period, x)
    assert close(-st.log_prob(x), S, 1e-6, atol=1e-5), worst(-st.log_prob(x), S, 1e-6)           # (float32 rows: 1 / period)
    t0 = fa.LatticeXY(shape, J, 0.0, period, use_gpu=False)                                      # O(2): a global rotation
    st0 = rc.RotorStatement(t0.site_rows, t0.table)
    assert close(st0.log_prob(x + 0.37 * period), st0.log_prob(x), 1e-6, atol=1e-5)
    for mu in range(len(shape)):                                                                 # lattice translations
        moved = torch.roll(x.reshape((7,) + tuple(shape)), 1, dims=mu + 1).reshape(7, D)
        assert close(st.log_prob(moved), st.log_prob(x), 1e-9, atol=1e-8)


def test_lattice_xy_metrics_and_refusals():
    fa = _targets()
    t = fa.LatticeXY((4, 4), 0.5, use_gpu=False)
    P = 2 * math.pi
    ordered, other = torch.full((1, 16), 0.3), torch.full((1, 16), 0.3 + P / 2)
    stripes = torch.zeros(1, 4, 4)
    stripes[:, :, 1::2] = P / 2                                                 # columns alternate: no net magnetisation
    x = torch.cat([ordered, other, stripes.reshape(1, 16)])
    m = t.performance_metrics(x, torch.log(torch.tensor([1.0, 1.0, 2.0], dtype=torch.float64)))
    # ordered rows: |m| = 1, every bond cosine 1; stripes: m = 0, bonds along a row -1, along a column +1 -> mean 0
    assert abs(m["abs_magnetisation"] - 0.5) < 1e-6 and abs(m["magnetisation_sq"] - 0.5) < 1e-6 and abs(m["neighbour_cosine"] - 0.5) < 1e-6
    with pytest.raises(ValueError, match="sites"):
        fa.LatticeXY((9, 8), 0.3, use_gpu=False)
    with pytest.raises(ValueError, match="positive extents"):
        fa.LatticeXY((4, 0), 0.3, use_gpu=False)
    one = fa.LatticeXY((1, 5), 0.3, use_gpu=False)                              # an extent of 1 is left out of the table
    assert one.n_neighbours == 2 and one.n_bonds == 5


# ---- the direct cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,density", rc.all_cases())
def test_float32_statement_stays_inside_a_quarter_of_the_tolerance_also_under_sixteen_ulp_nudges(D, density):
    c = rc.case(D, density)
    g = torch.Generator().manual_seed(5 + D)
    per = c["P"] > 0
    span = torch.where(per, 1.5 * c["P"], torch.full_like(c["P"], 3.0))
    assert float(c["P"][per].min()) >= 2.0 and float(c["P"].max()) <= 7.0
    assert float(c["rows"][:6].abs().max()) <= 1.0 and float(c["K32"].abs().max()) <= 0.5 / math.sqrt(c["NB"]) + 1e-7
    rows = [c["rows_x"]["wide"]] + [rc.nudged(c["rows_x"]["wide"], g) for _ in range(4)]
    for x in rows:
        assert bool((x.abs() <= span * (1 + 1e-5)).all())
        lp64, g64 = c["st64"].log_prob_and_grad(x)
        lp32, g32 = c["st32"].log_prob_and_grad(x.float())
        assert lp32.dtype == torch.float32 and g32.dtype == torch.float32
        print(f"MEASURE D={D} {density} NB={c['NB']} | fp32 statement | log p {worst(lp32, lp64):.3f} | grad {worst(g32, g64):.3f}")
        assert worst(lp32, lp64) < 0.25 and worst(g32, g64) < 0.25
    lp64, g64 = c["ref"]["special"]
    lp32, g32 = c["st32"].log_prob_and_grad(c["rows_x"]["special"].float())
    assert close(lp32, lp64) and close(g32, g64)             # (`close` asks for equal non-finite patterns)


@pytest.mark.parametrize("D,density,name", [(D, d, n) for D, d in rc.all_cases() for n, m in rc.MUTANTS.items() if m[2](D)])
def test_every_one_line_mutant_moves_a_compared_value_beyond_the_tolerance(D, density, name):
    cls, where, _ = rc.MUTANTS[name]               # (listed only where the mutant is not the statement itself: D = 1, D = 16)
    c = rc.case(D, density)
    x = c["rows_x"]["wide"]
    lp, g = cls(c["rows"], c["table"], log_norm=c["log_norm"]).log_prob_and_grad(x)
    lp64, g64 = c["ref"]["wide"]
    u_lp, u_g = mc.tol_units(lp[:, None], lp64[:, None]), mc.tol_units(g, g64)
    print(f"MEASURE D={D} {density} {name} | rows beyond the tolerance: log p {int((u_lp > 1).sum())}, grad {int((u_g > 1).sum())} of {x.shape[0]}")
    if where in ("both", "log_p"):
        assert float(u_lp.max()) > 100 and int((u_lp > 10).sum()) >= x.shape[0] // 4
    if where in ("both", "grad"):
        assert float(u_g.max()) > 100 and int((u_g > 10).sum()) >= x.shape[0] // 4
    if where == "log_p":
        assert torch.equal(g, g64)
    if where == "grad":
        assert torch.equal(lp, lp64)


# ---- the transition cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rc.T_SHAPES + rc.EXTRA_SHAPES, ids=str)
def test_no_accept_decision_of_a_transition_case_sits_inside_the_rounding_band(shape):
    c = rc.t_case(*shape)
    assert c["cap"] == 0 and torch.equal(c["cls32"], c["cls64"])
    acc = [float(a.float().mean()) for a in c["accept"]]
    assert all(0.15 < a < 0.98 for a in acc) and any(a < 0.95 for a in acc), acc
    o32, o64 = c["o32"], c["o64"]
    for k in ("x", "log_q", "log_p", "grad_log_p"):
        assert worst(getattr(o32, k), getattr(o64, k)) < 0.5, k
    assert worst(c["lw32"], c["lw64"]) < 0.5
    assert float(rc.perturbed_worst(*shape).max()) < 0.5
    per = c["P"] > 0
    assert 0 < int(per.sum()) < shape[0] and bool((c["K32"] != 0).any())
    if shape[1] == mc.SPLINE:                                  # the target sits on the flow's torus
        assert torch.nonzero(per).flatten().tolist() == sorted(mc.SPLINE_ARGS["circ"])
        assert torch.equal(c["P"][per], 2.0 * c["tail_bound"].double()[per])
    # the target matters to the case: with the sine terms' gradient sign wrong the chains end elsewhere
    out, _, start = rc.run_oracle(*shape, target_cls=rc.SineGradientPlus)
    assert int(rc.moved_chains(out, start, c).sum()) >= shape[3] // 4


def test_metropolis_case_conditions():
    c = rc.metropolis_case()
    assert c["cap"] == 0 and torch.equal(c["acc64"], c["acc32"])
    assert all(0.15 < float(a) < 0.9 for a in c["acc64"].float().mean(1))
    assert worst(c["o32"].x, c["o64"].x) < 0.5 and worst(c["lw32"], c["lw64"]) < 0.5


@pytest.mark.parametrize("shape,mix", [(s, False) for s in rc.CHAIN_SHAPES] + [(rc.MIX_SHAPE, True)], ids=str)
def test_whole_call_case_conditions(shape, mix):
    c = rc.chain_case(*shape, mix=mix)
    assert c["cap"] == 0 and torch.equal(c["dec32"], c["dec64"])
    assert 0.1 < float(c["dec64"].float().mean()) < 0.98
    p32, p64 = c["pt32"], c["pt64"]
    for k in ("x", "log_q", "log_p"):
        assert worst(getattr(p32, k), getattr(p64, k), M * 1e-4) < 0.5, k
    assert worst(c["lw32"], c["lw64"], M * 1e-4) < 0.5 and worst(p32.grad_log_q, p64.grad_log_q, M * 5e-4) < 0.5


# ---- the class -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,density", [(2, "dense"), (17, "sparse"), (64, "dense")])
def test_class_builds_the_statements_rows_and_table(D, density):
    fa = _targets()
    c = rc.case(D, density)
    t = fa.CoupledRotorEnergy(**_native_form(c), use_gpu=False)
    assert t.table.dtype == torch.float32 and torch.equal(t.table, c["table"]) and torch.equal(t.site_rows, c["rows"])
    assert t.n_neighbours == c["NB"] and t.dim == D
    # wrap: into [-P/2, P/2), line sites untouched, idempotent, and log p does not see it
    x = c["rows_x"]["wide"].float()
    y = t.wrap(x)
    per = c["P"] > 0
    half = (0.5 * c["P"]).float()
    assert torch.equal(y[:, ~per], x[:, ~per]) and bool((y[:, per] >= -half[per]).all() and (y[:, per] < half[per]).all())
    assert torch.equal(t.wrap(y), y)
    lp_x, lp_y = c["st64"].log_prob(x.double()), c["st64"].log_prob(y.double())
    assert close(lp_y, lp_x, 1e-5, atol=1e-4), worst(lp_y, lp_x, 1e-5)       # (y = x - n P rounded to float32)


def test_for_flow_shares_the_flows_torus():
    fa = _targets()
    D, circ = 7, (1, 4, 5)
    tb = torch.tensor([5.0, 1.5, 5.0, 5.0, math.pi, 2.25, 5.0])
    flow = fa.CircularCoupledRQSFlow(D, 2, 16, circ, tb)
    per = torch.zeros(D, dtype=torch.bool)
    per[list(circ)] = True
    A = torch.zeros(3, D, dtype=torch.float64)
    A[0, per] = 0.5
    K = torch.zeros(D, D, dtype=torch.float64)
    K[1, 4] = K[4, 1] = 0.3
    t = fa.CoupledRotorEnergy.for_flow(flow, A, torch.zeros(3, D), K, line_quadratic=(~per).double() * 0.5, use_gpu=False)
    assert torch.equal(t._P64, torch.where(per, 2.0 * tb.double(), torch.zeros(D, dtype=torch.float64)))
    with pytest.raises(ValueError, match="touches a site on the line"):
        K2 = K.clone()
        K2[0, 1] = K2[1, 0] = 0.1
        fa.CoupledRotorEnergy.for_flow(flow, A, torch.zeros(3, D), K2, line_quadratic=(~per).double() * 0.5, use_gpu=False)


def test_constructor_refuses_by_name():
    fa = _targets()
    D = 4
    P = torch.tensor([2.0, 3.0, 0.0, 4.0])
    A = torch.tensor([[0.5, 0.2, 0.0, -0.3]])
    B = torch.zeros(1, D)
    K = torch.zeros(D, D)
    K[0, 1] = K[1, 0] = 0.4
    l, q = torch.tensor([0.0, 0.0, 0.1, 0.0]), torch.tensor([0.0, 0.0, 0.5, 0.0])
    ok = fa.CoupledRotorEnergy(P, A, B, K, l, q, use_gpu=False)
    assert ok.dim == D and ok.table.dtype == torch.float32 and ok.site_rows.shape == (9, D) and ok.table.shape == (2, D)
    assert ok.table[0].tolist() == [1.0, 0.0, 2.0, 3.0] and torch.equal(ok.table[1], torch.tensor([0.4, 0.4, 0.0, 0.0]))
    assert ok.site_rows[6].tolist() == [0.5, float(np.float32(1 / 3)), 0.0, 0.25]
    z = lambda n: torch.zeros(n)                               # noqa: E731
    Kn, Kd, Kl = torch.triu(torch.ones(D, D), 1) * (P > 0)[:, None] * (P > 0)[None], K.clone(), K.clone()
    Kd[0, 0] = 0.1
    Kl[2, 3] = Kl[3, 2] = 0.1
    bad = [("above the 64", (torch.ones(65), z(65), z(65), torch.zeros(65, 65))),
           ("must be", (P, A[:, :3], B, K, l, q)), ("must be", (P, A, B, torch.zeros(D, D + 1), l, q)),
           ("must be", (P, torch.zeros(4, D), torch.zeros(4, D), K, l, q)), ("must be", (P, A, B, K, l[:3], q)),
           ("period must be", (torch.zeros(0), z(0), z(0), torch.zeros(0, 0))), ("period must be", (torch.ones(2, 2), A, B, K)),
           ("not finite", (P, torch.tensor([[0.5, float("nan"), 0.0, 0.0]]), B, K, l, q)),
           ("not finite", (torch.tensor([2.0, float("inf"), 0.0, 4.0]), A, B, K, l, q)),
           ("not finite", (P, A, B, K, l, torch.tensor([0.0, 0.0, float("inf"), 0.0]))),
           ("negative", (torch.tensor([2.0, -3.0, 0.0, 4.0]), A, B, K, l, q)),
           ("not symmetric", (P, A, B, Kn, l, q)),
           ("non-zero diagonal", (P, A, B, Kd, l, q)),
           ("touches a site on the line", (P, A, B, Kl, l, q)),
           ("set on a periodic site", (P, A, B, K, torch.tensor([0.1, 0.0, 0.1, 0.0]), q)),
           ("set on a periodic site", (P, A, B, K, l, torch.tensor([0.0, 0.0, 0.5, 0.5]))),
           ("set on a site on the line", (P, torch.tensor([[0.5, 0.2, 0.1, -0.3]]), B, K, l, q)),
           ("set on a site on the line", (P, torch.cat([A, B]), torch.tensor([[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.2, 0.0]]), K, l, q)),
           ("must be > 0 on a site on the line", (P, A, B, K, l, z(D))),
           ("must be > 0 on a site on the line", (P, A, B, K, l, torch.tensor([0.0, 0.0, -0.5, 0.0])))]
    for match, args in bad:
        with pytest.raises(ValueError, match=match):
            fa.CoupledRotorEnergy(*args, use_gpu=False)
    # symmetric to 1e-6 of the largest entry is taken, and stored as (K + K^T) / 2
    Ks = torch.zeros(D, D, dtype=torch.float64)
    Ks[0, 1], Ks[1, 0] = 1.0, 1.0 + 5e-7
    t = fa.CoupledRotorEnergy(P, A, B, Ks, l, q, use_gpu=False)
    assert float(t._K64[0, 1]) == float(t._K64[1, 0]) == 1.0 + 2.5e-7
