"""The conditions test_gpu_hmc_mass.py relies on, asserted from the oracle alone (no GPU): the clamp of every case of
hmc_mass_cases.py binds on both sides and leaves most components free, both accept outcomes occur, the float32 oracle stays
inside the tolerance of the float64 one with at most one accept decision inside the rounding band (that count is the GPU test's
cap: a condition on the inputs, not a tolerance), every one-line mutant of the mass / clamp convention is far outside the
tolerance, and the three special rows (+inf, -inf, NaN in the start gradient) do what the reference does with them."""
import numpy as np
import pytest
import torch

import hmc_mass_cases as mc
from helpers import close, worst, RTOL
from oracle import ais as oais

CASES = mc.all_cases()
SP = list(mc.SPECIAL_ROWS)


def test_mass_vectors_are_distinct_per_component_and_per_lane():
    for D, K, nodes, B in mc.SHAPES:
        m = mc.inputs(D, K, nodes, B)["mass"]
        assert m.dtype == torch.float32 and m.shape == (D,) and len(set(m.tolist())) == D
        assert float(m.min()) >= 0.3 * (1 - 1e-6) and float(m.max()) <= 3.0 * (1 + 1e-6)
        assert all(m[j] != m[j + 16] for j in range(D - 16))
        if D == 60:                                          # four coordinates per lane, four different masses
            assert all(len({float(m[c + 16 * k]) for k in range(4) if c + 16 * k < D}) == len(range(c, D, 16)) for c in range(16))
        js = mc.special_coords(D)
        assert len(set(js)) == 3 and (D <= 17 or any(j >= 16 for j in js))
    assert {s[:3] for s in mc.SHAPES} == set(mc.TILES) and {s[:3] for s in mc.SHAPES + mc.EXTRA_SHAPES} == set(mc.PARAMS)


@pytest.mark.parametrize("D,K,nodes,B,kind", CASES)
def test_the_clamp_binds_on_both_sides_and_both_accept_outcomes_occur(D, K, nodes, B, kind):
    c = mc.case(D, K, nodes, B, kind)
    up, down, free = c["shares"]
    acc = [float(a.double().mean()) for a in c["accept"]]
    print(f"max_grad {c['max_grad']:.4f}: {up:.3f} at +max_grad, {down:.3f} at -max_grad, {free:.3f} free; accepted {acc}, "
          f"p_accept {c['p_accept']}")
    assert c["max_grad"] == float(np.float32(c["max_grad"])) and c["max_grad"] < 1e3
    assert up >= 0.05 and down >= 0.05 and free >= 0.30
    for a in acc:                                             # per outer step
        assert 0.25 <= a <= 0.90
    assert all(torch.isfinite(t).all() for t in (c["o64"].x, c["o64"].log_q, c["o64"].log_p, c["lw64"]))
    # the special rows accept (their exponential noise is SPECIAL_NOISE_E): a rejected row would hide its first half step
    assert bool((c["cls64"][SP] != 0).all())
    assert bool((c["noise_e"][:, SP] == mc.SPECIAL_NOISE_E).all())


@pytest.mark.parametrize("D,K,nodes,B,kind", CASES)
def test_float32_oracle_stays_inside_the_tolerance_of_the_float64_one(D, K, nodes, B, kind):
    c = mc.case(D, K, nodes, B, kind)
    o64, o32 = c["o64"], c["o32"]
    differ = c["cls64"] != c["cls32"]
    assert not bool((differ & ~c["in_band"]).any()), "the float32 oracle takes another decision outside the rounding band"
    assert c["cap"] <= 1, f"{c['cap']} rows inside the rounding band: pick another seed"
    assert int(differ.sum()) <= c["cap"]
    same = ~differ
    for k, a, b, rtol in (("x", o32.x, o64.x, RTOL), ("log_q", o32.log_q, o64.log_q, RTOL), ("log_p", o32.log_p, o64.log_p, RTOL),
                          ("log_w", c["lw32"], c["lw64"], RTOL), ("grad_log_q", o32.grad_log_q, o64.grad_log_q, 5e-4)):
        if k == "grad_log_q" and K == mc.SPLINE:              # (a spline knot: test_gpu_spline.py's transition test leaves it out too)
            continue
        print(f"{k}: fp32 oracle {worst(a[same], b[same], rtol):.2f} tolerance units")
        assert close(a[same], b[same], rtol), (k, worst(a[same], b[same], rtol))


@pytest.mark.parametrize("D,K,nodes,B", sorted({t[:4] for t in mc.TUNED}))
def test_step_size_targets_lie_below_and_above_every_acceptance_rate(D, K, nodes, B):
    """the step-size rule of the GPU test: with tuning on the second outer step runs on the adapted common step size; the two
    targets lie below / above every acceptance rate that run sees, and the float32 and float64 oracle agree on the decisions."""
    c = mc.case(D, K, nodes, B, "vector")
    for target in (mc.TARGET_LOW, mc.TARGET_HIGH):
        t32, t64 = (mc.tuned(D, K, nodes, B, "vector", target, dt) for dt in (torch.float32, torch.float64))
        for t in (t32, t64):
            assert all(mc.TARGET_LOW < p < mc.TARGET_HIGH for p in t["p_accept"]), t["p_accept"]
        up = target == mc.TARGET_LOW
        assert bool((t32["epsilons"] > c["eps"]).all()) == up and bool((t32["epsilons"] < c["eps"]).all()) == (not up)
        assert int((t32["cls"] != t64["cls"]).sum()) <= t64["cap"] <= 1


@pytest.mark.parametrize("D,K,nodes,B,kind", CASES)
def test_every_mutant_is_far_outside_the_tolerance(D, K, nodes, B, kind):
    c = mc.case(D, K, nodes, B, kind)
    for name, (cls, rows, applies) in mc.MUTANTS.items():
        if not applies(D) or (kind == "scalar" and cls is mc.LaneIndexedMass):
            continue
        out, _ = mc.run_oracle(D, K, nodes, B, c["mass_init"], torch.float64, cls=cls)
        moved = mc.moved_rows(out, mc.log_w_after(out, c["lw_in"]), c)
        print(f"{name}: {int(moved.sum())} of {B} chains more than 100 tolerances away")
        if K == mc.SPLINE and cls in (mc.KineticWithoutMass, mc.KineticTimesMass):
            # The spline case's own criterion for the two mutants that change DECISIONS only (same trajectory, another
            # acceptance quantity): at its step size the energy error is small and few of its 20 chains sit close enough to
            # the threshold to flip.  What the GPU test (cap 0: every decision must be float64's) needs is that the mutant's
            # log-acceptance is far from the oracle's in units of the rounding band on a quarter of the chains, and that at
            # least one chain does flip.
            far = (_.last_margin - c["h64"].last_margin).abs() > 100 * c["band"]
            print(f"{name}: margin more than 100 bands away on {int(far.sum())} chains")
            assert float(far.double().mean()) >= 0.25 and int(moved.sum()) >= 1, (name, int(far.sum()), int(moved.sum()))
        elif rows == "quarter":
            assert float(moved.double().mean()) >= 0.25, (name, int(moved.sum()))
        else:                                                 # the +inf and the -inf row (NaN -> 0 either way)
            assert bool(moved[SP[:2]].all()), (name, moved[SP].tolist())


@pytest.mark.parametrize("D,K,nodes,B,mix", [s + (False,) for s in mc.CHAIN_SHAPES] + [mc.MIX_SHAPE + (True,)])
def test_whole_call_cases(D, K, nodes, B, mix):
    """The free-running call of M_CHAIN transitions (and the one over the defensive mixture): the clamp binds, both outcomes occur,
    no chain is filtered, at most one row has a decision inside the rounding band, and the float32 oracle stays inside M x the
    tolerance of the float64 one on every row whose decisions agree."""
    c = mc.chain_case(D, K, nodes, B, mix=mix)
    up, down, free = c["shares"]
    acc = float(c["dec64"].double().mean())
    print(f"{up:.3f} at +max_grad, {down:.3f} at -max_grad, {free:.3f} free; {acc:.3f} of the {c['dec64'].numel()} decisions accept")
    assert up >= 0.05 and down >= 0.05 and free >= 0.30 and 0.25 <= acc <= 0.90
    assert c["cap"] <= 1
    same = (c["dec64"] == c["dec32"]).all(0)
    assert not bool((~same & ~c["in_band"]).any()) and int((~same).sum()) <= c["cap"]
    FR, M = mc.M_CHAIN * RTOL, mc.M_CHAIN
    for k, a, b in (("x", c["pt32"].x, c["pt64"].x), ("log_q", c["pt32"].log_q, c["pt64"].log_q), ("log_p", c["pt32"].log_p, c["pt64"].log_p),
                    ("log_w", c["lw32"], c["lw64"])):
        print(f"{k}: fp32 oracle {worst(a[same], b[same], FR):.2f} tolerance units")
        assert close(a[same], b[same], FR, atol_scale=M), (k, worst(a[same], b[same], FR))
    if mix:                                                   # both branches of the mixture start chains
        branch = c["sel"] < torch.sigmoid(torch.tensor(mc.MIX_LOGIT))
        assert 0 < int(branch.sum()) < B


@pytest.mark.parametrize("D,K,nodes,B", mc.SHAPES)
def test_special_rows_first_half_step(D, K, nodes, B):
    """hmc.py:194-199 on the start point: g = -(g_q grad_log_q + g_p grad_log_p) with g_p > 0, so +inf in grad_log_p is -inf in
    grad U -> -max_grad, -inf -> +max_grad, NaN -> 0; every other entry of grad U is what the un-injected point gives."""
    c = mc.inputs(D, K, nodes, B)
    h = oais.HMC(1, D, None, None, alpha=mc.ALPHA, p_target=False, max_grad=c["max_grad"], dtype=torch.float64)
    with_v, without = h._grad_U(c["start"], mc.BETA), h._grad_U(c["plain"], mc.BETA)
    expect = without.clone()
    for r, j, v in zip(SP, mc.special_coords(D), (-c["max_grad"], c["max_grad"], 0.0)):
        expect[r, j] = v
    assert torch.equal(with_v, expect)
    # ... and the half step p - eps grad U / 2 of those rows moves by exactly that much
    eps = float(c["eps"][0, 0] + c["ceps"][0])
    p0 = c["noise_p"][0].double() * c["mass"].double()
    d = (p0 - eps * with_v / 2) - (p0 - eps * without / 2)
    for r, j, v in zip(SP, mc.special_coords(D), (-c["max_grad"], c["max_grad"], 0.0)):
        assert abs(float(d[r, j]) - (-eps * (v - float(without[r, j])) / 2)) <= 1e-12
        mask = torch.ones_like(d, dtype=torch.bool)
        mask[r, j] = False
        assert float(d[r][mask[r]].abs().max()) == 0.0


def test_hooked_oracle_equals_the_written_out_transition():
    """oracle.ais.HMC routes the three uses of the mass through `_momentum`, `_position`, `_kinetic`: the same expressions as
    the loop written out (hmc.py:134, :142, :126-127), bit for bit."""
    D, K, nodes, B = mc.SHAPES[0]
    c = mc.case(D, K, nodes, B, "vector")
    m, mg, dt = c["mass"].double(), c["max_grad"], torch.float64
    nf, tgt = c["nf64"], c["tgt"]
    point = current = mc._point_to(c["start"], dt)

    def grad_u(pt):
        g = -oais.grad_intermediate_log_prob(pt, mc.BETA, mc.ALPHA, False)
        return torch.nan_to_num(torch.clamp(g, max=mg, min=-mg), nan=0.0, posinf=0.0, neginf=0.0)
    for n in range(mc.N_OUTER):
        eps = c["eps"].double()[0, n] + c["ceps"].double()
        p = c["noise_p"][n].double() * m
        p_cur = p
        gu = grad_u(point)
        for _ in range(c["L"]):
            p = p - eps * gu / 2
            point = oais.create_point(point.x + eps / m * p, nf.log_prob, tgt.log_prob, with_grad=True)
            gu = grad_u(point)
            p = p - eps * gu / 2
        la = (oais.intermediate_log_prob(point, mc.BETA, mc.ALPHA, False) - torch.sum(p ** 2 / m, -1) / 2) - \
            (oais.intermediate_log_prob(current, mc.BETA, mc.ALPHA, False) - torch.sum(p_cur ** 2 / m, -1) / 2)
        accept = (torch.nan_to_num(la, nan=-float("inf"), posinf=-float("inf"), neginf=-float("inf")) > -c["noise_e"][n].double()) \
            & torch.isfinite(la)
        assert torch.equal(accept, c["accept"][n])
        current[accept] = point[accept]
    assert torch.equal(current.x, c["o64"].x) and torch.equal(current.log_q, c["o64"].log_q)
