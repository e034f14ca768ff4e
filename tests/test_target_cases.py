"""The conditions test_gpu_targets.py relies on, asserted from the restatements of target_cases.py alone (no GPU): the
statements are the oracle's targets (which fixture g3 pins to the reference) with the gradient written out; the scales of every
GMM case tell a wrong index from the right one; the float32 statement stays inside `helpers.close` of the float64 one on every
group of rows; the rows reach what they are listed for (two live components, every lane slot, both sides of the mask); every
transition case accepts 25 - 90 % per outer step with at most one decision inside the rounding band (the GPU test's cap: a
condition on the inputs, not a tolerance); and every one-line mutant is >= 100 tolerances away on >= 25 % of the rows of some
group, or of the chains of every transition case where it can differ."""
import math

import pytest
import torch

import hmc_mass_cases as mc
import target_cases as tc
from helpers import close, worst, RTOL
from oracle import ais as oais
from oracle import targets as otgt

GMM_CASES = tc.all_gmm_cases()
FACTOR, SHARE = 100.0, 0.25
# The transition cases leave the float32 oracle a QUARTER of the tolerance: a leapfrog trajectory amplifies rounding, a kernel sums
# in another order than torch (sequentially over D, where torch adds pairwise), and the float32 oracle itself lands elsewhere on
# another CPU.  A case whose float32 oracle sits at 0.9 tolerances says nothing about a kernel that is 1.3 away.
QUARTER = 0.25


def _autograd(fn, x):
    x = x.clone().requires_grad_(True)
    lp = fn(x)
    return lp.detach(), torch.autograd.grad(lp, x, torch.ones_like(lp))[0]


def _same_nonfinite(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.where(torch.isinf(a), a, torch.zeros_like(a)),
                                                                      torch.where(torch.isinf(b), b, torch.zeros_like(b)))


# ---- the statements are the oracle's targets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n_mix,reference", GMM_CASES)
def test_gmm_statement_is_the_oracle_gmm_with_its_gradient_written_out(D, n_mix, reference):
    c = tc.gmm_case(D, n_mix, reference)
    o = otgt.GMM(D, n_mix, locs=c["locs"].double(), scales=c["scales"].double())
    if reference:                                             # ... and that constructor argument changes nothing of the seeded one
        seeded = otgt.GMM(*tc.REFERENCE_CASE)
        assert torch.equal(seeded.locs, c["locs"]) and torch.equal(seeded.scales, c["scales"]) and len(set(c["scales"].reshape(-1).tolist())) == 1
    for name, x in c["rows"].items():
        lp, g = c["st64"].log_prob_and_grad(x)
        lp_o, g_o = _autograd(o.log_prob, x)
        assert _same_nonfinite(lp, lp_o) and _same_nonfinite(g, g_o), name
        assert close(lp, lp_o, 1e-12, atol=1e-9) and close(g, g_o, 1e-10, atol=1e-9), name
        # the autograd node of the statement hands out the written-out gradient
        assert torch.equal(_autograd(c["st64"].log_prob, x)[1].nan_to_num(nan=7.0), g.nan_to_num(nan=7.0))
    lp, g = c["st64"].log_prob_and_grad(c["rows"]["special"])
    assert torch.isnan(lp[0]) and lp[1] == -tc.INF and torch.isfinite(lp[2])
    assert bool(torch.isnan(g[:2]).all()) and bool(torch.isfinite(g[2]).all())


@pytest.mark.parametrize("D", tc.MW_DIMS)
def test_manywell_statement_is_the_oracle_manywell(D):
    rows = tc.manywell_rows(D)
    for name, x in rows.items():
        for normalised in (False, True):
            o = otgt.ManyWell(D, normalised=normalised)
            st = tc.manywell_statement(D, tc.DEFAULT_ABC, "log_Z" if normalised else "zero")
            lp, g = st.log_prob_and_grad(x)
            lp_o = o.log_prob(x)
            assert _same_nonfinite(lp, lp_o) and close(lp, lp_o, 1e-12, atol=1e-9), name
            if name != "special":
                assert close(g, o.grad_log_prob(x), 1e-12, atol=1e-9) and close(g, _autograd(o.log_prob, x)[1], 1e-10, atol=1e-9)
        o = otgt.ManyWell(D, *tc.MW_ABC[1])
        assert close(tc.manywell_statement(D, tc.MW_ABC[1], "zero").log_prob_and_grad(x)[0], o.log_prob(x), 1e-12, atol=1e-9)
    assert float(rows["wide"].abs().max()) == 4.0 and float(rows["wide"].min()) == -4.0


# ---- the GMM cases -----------------------------------------------------------------------------------------------------------------
def test_the_shapes_cover_every_lane_count_and_every_coordinate_count():
    Ds, ns = {s[0] for s in tc.GMM_SHAPES}, {s[1] for s in tc.GMM_SHAPES}
    assert {1, 3, 5, 7, 16, 17, 33, 40, 50, 64} <= ns and {16, 33, 60, 64} <= Ds
    assert any(D < 16 for D in Ds) and any(17 <= D <= 32 for D in Ds) and max(Ds) == 64       # 64 = FABHIP_MAX_DIM
    assert {s[:3] for s in tc.T_SHAPES} == set(tc.T_TILES) and {s[:3] for s in tc.T_SHAPES} >= {s[:3] for s in mc.SHAPES}
    assert (2, 2, 40) in tc.T_TILES and dict((s[:3], s[4]) for s in tc.T_SHAPES)[(2, 2, 40)] == 5
    assert tc.METROPOLIS_SHAPE[0] == 5 and tc.METROPOLIS_SHAPE[4] == 17


@pytest.mark.parametrize("D,n_mix", tc.GMM_SHAPES)
def test_scales_tell_a_wrong_index_from_the_right_one(D, n_mix):
    s = tc.gmm_case(D, n_mix)["scales"]
    assert s.dtype == torch.float32 and s.shape == (n_mix, D) and len(set(s.reshape(-1).tolist())) == n_mix * D
    assert float(s.min()) >= 0.4 * (1 - 1e-6) and float(s.max()) <= 1.6 * (1 + 1e-6)
    if D > 1:
        assert bool((s[:, 1:] != s[:, :1]).all())                                      # scales[k][j] != scales[k][0]
    if n_mix > 1:
        assert bool((s[1:] != s[:1]).all())                                            # != scales[0][j]
    if D > 1 and n_mix > 1:
        flat_same = (torch.arange(n_mix)[:, None] * D + torch.arange(D)[None]) == \
            (torch.arange(D)[None] * n_mix + torch.arange(n_mix)[:, None])               # entries a transposed read leaves in place
        assert bool((s != s.T.reshape(n_mix, D))[~_fixed_by_transpose(n_mix, D)].all())
        assert bool((s != s.reshape(D, n_mix).T)[~flat_same].all())


def _fixed_by_transpose(n_mix, D):
    """entries [k, j] of s.T.reshape(n_mix, D) that are the entry [k, j] of s itself"""
    idx = torch.arange(n_mix * D).reshape(n_mix, D)
    return idx.T.reshape(n_mix, D) == idx


@pytest.mark.parametrize("D,n_mix,reference", GMM_CASES)
def test_float32_statement_is_inside_the_tolerance_on_every_group_and_the_rows_reach_their_branches(D, n_mix, reference):
    c = tc.gmm_case(D, n_mix, reference)
    slots = set()
    for name in tc.GROUPS:
        x = c["rows"][name]
        assert x.shape == (tc.B_ROWS, D) and torch.equal(x, x.float().double())
        lp64, g64, w, raw = c["ref"][name]
        lp32, g32 = c["st32"].log_prob_and_grad(x.float())
        print(f"{name}: fp32 statement log p {worst(lp32, lp64):.2f}, gradient {worst(g32, g64):.2f} tolerance units; "
              f"log p in [{float(raw.min()):.0f}, {float(raw.max()):.0f}]")
        assert close(lp32, lp64) and close(g32, g64), (name, worst(lp32, lp64), worst(g32, g64))
        slots |= set((w.argmax(-1) % 16).tolist())
        second = w.sort(-1).values[:, -2] if n_mix > 1 else torch.zeros(tc.B_ROWS, dtype=torch.float64)
        if name == "between" and n_mix > 1:
            assert float((second > 0.05).double().mean()) >= 0.25 and float(raw.min()) > -1e3         # near field only
        if name == "far":
            masked = raw < tc.MASK
            assert bool((second < 1e-3).all()) and bool(((raw - tc.MASK).abs() > 0.01 * abs(tc.MASK)).all())
            assert int(masked.sum()) >= 2 and int((~masked & (raw < -5000)).sum()) >= 2 and float(raw.max()) > -2.6 * max(D, 12)
            assert float(masked.double().mean()) >= SHARE     # (the mutant that zeroes the gradient there shows on a quarter)
            assert torch.equal(lp64 == -tc.INF, masked) and bool(torch.isfinite(g64).all())
            for B in (15, 16, 17):                            # live and masked rows side by side in every slice the GPU test takes
                assert 0 < int(masked[:B].sum()) < B
    assert slots == set(range(min(n_mix, 16))), slots


# ---- GMM mutants on the rows ------------------------------------------------------------------------------------------------------
def _moved(st, c, name):
    """(share of rows of group `name` moved in log p, share moved in the gradient) by more than FACTOR tolerances"""
    lp64, g64 = c["ref"][name][:2]
    lp, g = st.log_prob_and_grad(c["rows"][name])
    fin = torch.isfinite(lp64)
    ulp = torch.zeros(lp64.shape[0], dtype=torch.float64)
    if fin.any():
        ulp[fin] = mc.tol_units(lp[fin][:, None], lp64[fin][:, None])
    ulp[torch.isfinite(lp) != fin] = float("inf")
    return float((ulp > FACTOR).double().mean()), float((tc.grad_units(g, g64) > FACTOR).double().mean())


@pytest.mark.parametrize("mutant", list(tc.GMM_MUTANTS))
def test_every_gmm_mutant_is_far_outside_the_tolerance_where_it_can_differ(mutant):
    cls, shows_at, applies, _ = tc.GMM_MUTANTS[mutant]
    for D, n_mix in tc.GMM_SHAPES:
        shows = shows_at
        c = tc.gmm_case(D, n_mix)
        st = cls(c["locs"], c["scales"])
        shares = {name: _moved(st, c, name) for name in tc.GROUPS}
        print(f"{mutant} at ({D}, {n_mix}): " + ", ".join(f"{n} {a:.2f} / {b:.2f}" for n, (a, b) in shares.items()))
        if not applies(D, n_mix):                             # ... and is the statement itself where it cannot
            for name in tc.GROUPS:
                lp, g = st.log_prob_and_grad(c["rows"][name])
                assert torch.equal(lp, c["ref"][name][0]) and torch.equal(g, c["ref"][name][1]), (mutant, D, n_mix, name)
            continue
        best_lp, best_g = max(a for a, _ in shares.values()), max(b for _, b in shares.values())
        if mutant == "hld dropped" and n_mix == 1:            # (one component: its half log determinant is a constant of log p)
            shows = "log_p"
        if shows == "log_p":                                  # a constant of log p: no gradient moves
            assert best_lp >= SHARE and best_g == 0.0, (mutant, D, n_mix, shares)
        elif shows == "grad":
            assert best_g >= SHARE and best_lp == 0.0, (mutant, D, n_mix, shares)
        else:
            assert best_g >= SHARE, (mutant, D, n_mix, shares)


# ---- ManyWell ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,abc,which", tc.all_manywell_cases())
def test_manywell_float32_statement_and_mutants(D, abc, which):
    rows = tc.manywell_rows(D)
    st64, st32 = tc.manywell_statement(D, abc, which), tc.manywell_statement(D, abc, which, torch.float32)
    for name in ("wide", "modes", "special"):
        x = rows[name]
        lp64, g64 = st64.log_prob_and_grad(x)
        lp32, g32 = st32.log_prob_and_grad(x.float())
        assert close(lp32, lp64) and close(g32, g64), (name, worst(lp32, lp64), worst(g32, g64))
    sp, gsp = st64.log_prob_and_grad(rows["special"])
    assert not bool(torch.isfinite(sp).any()) and int((~torch.isfinite(gsp)).sum()) == 6      # one coordinate per special row
    for mutant, (cls, shows) in tc.MANYWELL_MUTANTS.items():
        st = tc.manywell_statement(D, abc, which, cls=cls)
        best_lp = best_g = 0.0
        for name in ("wide", "modes"):
            lp64, g64 = st64.log_prob_and_grad(rows[name])
            lp, g = st.log_prob_and_grad(rows[name])
            best_lp = max(best_lp, float((mc.tol_units(lp[:, None], lp64[:, None]) > FACTOR).double().mean()))
            best_g = max(best_g, float((mc.tol_units(g, g64) > FACTOR).double().mean()))
        print(f"{mutant}: log p {best_lp:.2f}, gradient {best_g:.2f} of the rows of its best group")
        if mutant == "+ log_norm":
            if which == "zero":
                assert best_lp == 0.0 and best_g == 0.0
            else:                                             # 2 log_norm against |log p| of the rows around the wells
                assert best_g == 0.0 and (best_lp >= SHARE or D > tc.LOG_NORM_SHOWS_UP_TO), (mutant, best_lp)
        elif shows == "grad":
            assert best_g >= SHARE and best_lp == 0.0
        else:
            assert best_g >= SHARE and best_lp >= SHARE


def test_the_log_norm_mutant_shows_at_every_constant_on_some_dimension():
    for abc in tc.MW_ABC:
        for which in tc.MW_LOG_NORMS[1:]:
            shares = []
            for D in tc.MW_DIMS:
                x = tc.manywell_rows(D)["modes"]
                lp64 = tc.manywell_statement(D, abc, which).log_prob_and_grad(x)[0]
                lp = tc.manywell_statement(D, abc, which, cls=tc.LogNormAdded).log_prob_and_grad(x)[0]
                shares.append(float((mc.tol_units(lp[:, None], lp64[:, None]) > FACTOR).double().mean()))
            assert all(sh >= SHARE for D, sh in zip(tc.MW_DIMS, shares) if D <= tc.LOG_NORM_SHOWS_UP_TO), (abc, which, shares)


# ---- transition cases -------------------------------------------------------------------------------------------------------------
T_ALL = tc.T_SHAPES + tc.EXTRA_SHAPES + [tc.MW_T_SHAPE]


@pytest.mark.parametrize("D,K,nodes,B,n_mix", T_ALL)
def test_transition_cases_accept_a_share_and_float32_stays_inside_the_tolerance(D, K, nodes, B, n_mix):
    c = tc.t_case(D, K, nodes, B, n_mix)
    acc = [float(a.double().mean()) for a in c["accept"]]
    s = c["scales"]
    print(f"accepted {acc}, p_accept {c['p_accept']}, start log p in [{float(c['start'].log_p.min()):.0f}, {float(c['start'].log_p.max()):.0f}]")
    for a in acc:
        assert 0.25 <= a <= 0.90
    if n_mix != tc.MW:
        assert len(set(s.reshape(-1).tolist())) == n_mix * D and bool((s[:, 1:] != s[:, :1]).all()) and bool((s[1:] != s[:1]).all())
        # the means lie inside the flow's sample spread: no further out than its own samples
        assert float(c["locs"].abs().max()) <= 2.0 * float(c["start"].x.abs().max())
    o64, o32 = c["o64"], c["o32"]
    assert all(torch.isfinite(t).all() for t in (o64.x, o64.log_q, o64.log_p, o64.grad_log_p, c["lw64"]))
    differ = c["cls64"] != c["cls32"]
    assert not bool((differ & ~c["in_band"]).any()) and c["cap"] <= 1 and int(differ.sum()) <= c["cap"]
    same = ~differ
    for k, a, b, rtol in (("x", o32.x, o64.x, RTOL), ("log_q", o32.log_q, o64.log_q, RTOL), ("log_p", o32.log_p, o64.log_p, RTOL),
                          ("log_w", c["lw32"], c["lw64"], RTOL), ("grad_log_p", o32.grad_log_p, o64.grad_log_p, RTOL),
                          ("grad_log_q", o32.grad_log_q, o64.grad_log_q, 5e-4)):
        if k == "grad_log_q" and K == mc.SPLINE:              # (a spline knot: test_gpu_spline.py's transition test leaves it out too)
            continue
        print(f"{k}: fp32 oracle {worst(a[same], b[same], rtol):.2f} tolerance units")
        assert close(a[same], b[same], rtol) and worst(a[same], b[same], rtol) <= QUARTER, (k, worst(a[same], b[same], rtol))
    assert float(c["lw64"].abs().max()) < 1e3 and float(o64.x.abs().max()) < 1e2          # no chain has left the flow's range
    if K != mc.SPLINE:                                        # (a knot is the spline test's own allowance)
        nudged = tc.perturbed_worst(D, K, nodes, B, n_mix)
        print(f"float32 oracle under nudged starts: worst chain {float(nudged.max()):.2f} tolerance units in x and grad_log_p")
        assert float(nudged.max()) <= 1.0, nudged.tolist()


@pytest.mark.parametrize("D,K,nodes,B,n_mix", tc.T_SHAPES)
def test_every_gmm_mutant_moves_a_quarter_of_the_chains_of_every_transition_case(D, K, nodes, B, n_mix):
    c = tc.t_case(D, K, nodes, B, n_mix)
    for mutant, (cls, shows, applies, needs_masked) in tc.GMM_MUTANTS.items():
        if needs_masked or not applies(D, n_mix):             # (no chain of a transition case is masked)
            continue
        out, _, start = tc.run_oracle(D, K, nodes, B, n_mix, torch.float64, cls)
        moved = tc.moved_chains(out, start, c)
        x_moved = mc.tol_units(out.x, c["o64"].x) > FACTOR
        print(f"{mutant}: {int(moved.sum())} of {B} chains more than 100 tolerances away ({int(x_moved.sum())} in x)")
        assert float(moved.double().mean()) >= SHARE, (mutant, int(moved.sum()))
        if shows == "log_p":                                  # a constant of log p: the trajectory and every decision stay
            assert int(x_moved.sum()) == 0


def test_metropolis_case():
    c = tc.metropolis_case()
    D, K, nodes, B, n_mix = tc.METROPOLIS_SHAPE
    acc = c["acc64"].double().mean(1).tolist()
    print(f"accepted {acc}; {c['cap']} rows inside the band")
    assert all(0.25 <= a <= 0.90 for a in acc) and c["cap"] <= 1
    differ = (c["acc64"] != c["acc32"]).any(0)
    assert not bool((differ & ~c["in_band"]).any()) and int(differ.sum()) <= c["cap"]
    same = ~differ
    for k, a, b in (("x", c["o32"].x, c["o64"].x), ("log_q", c["o32"].log_q, c["o64"].log_q), ("log_p", c["o32"].log_p, c["o64"].log_p),
                    ("log_w", c["lw32"], c["lw64"])):
        assert close(a[same], b[same]), (k, worst(a[same], b[same]))
    for mutant, (cls, shows, applies, needs_masked) in tc.GMM_MUTANTS.items():
        if needs_masked or shows == "grad" or not applies(D, n_mix):         # (Metropolis takes no gradient)
            continue
        out = c["run"](torch.float64, cls)[0]
        moved = (mc.tol_units(out.x, c["o64"].x) > FACTOR) | (mc.tol_units(out.log_p[:, None], c["o64"].log_p[:, None]) > FACTOR)
        print(f"{mutant}: {int(moved.sum())} of {B} chains")
        assert float(moved.double().mean()) >= SHARE, (mutant, int(moved.sum()))


@pytest.mark.parametrize("D,K,nodes,B,n_mix,mix", [s + (False,) for s in tc.CHAIN_SHAPES] + [tc.MIX_SHAPE + (True,)])
def test_whole_call_cases(D, K, nodes, B, n_mix, mix):
    """hmc_mass_cases' conditions for a free-running call of M transitions, on the float64 run: both outcomes occur, no chain is
    filtered or leaves the flow's range, at most one row has a decision inside the band."""
    c = tc.chain_case(D, K, nodes, B, n_mix, mix=mix)
    acc = float(c["dec64"].double().mean())
    print(f"{acc:.3f} of the {c['dec64'].numel()} decisions accept, cap {c['cap']}")
    assert 0.25 <= acc <= 0.90 and c["cap"] <= 1
    # The float32 run of a free-running call is printed, not asserted: three transitions compound its rounding, and where it lands
    # depends on the CPU and the torch build (the same case holds 0.06 tolerances in x on one machine and leaves float64 on another).
    # The GPU file compares with float64 alone; what the case owes it is stated on the float64 run.
    same = (c["dec64"] == c["dec32"]).all(0)
    FR = tc.M_CHAIN * RTOL
    print(f"float32 oracle: {int((~same).sum())} chains take another decision; x {worst(c['pt32'].x[same], c['pt64'].x[same], FR):.2f}, "
          f"log_w {worst(c['lw32'][same], c['lw64'][same], FR):.2f} tolerance units on the others")
    # every chain stays in the flow's range in float64 (a chain that runs away has a log-weight of 1e100 and no margin to speak of)
    assert bool(torch.isfinite(c["lw64"]).all()) and float(c["lw64"].abs().max()) < 1e3 and float(c["pt64"].x.abs().max()) < 1e2
    # (a proposal that overflows has a NaN or infinite log-acceptance and is rejected, hmc.py:151-153, and the reference starts the
    # next outer step from it: such decisions are part of the cases, and none of them is "inside the band")
    print(f"{int((~torch.isfinite(c['margins'])).sum())} of {c['margins'].numel()} decisions reject a non-finite proposal")
