"""The conditions test_gpu_metropolis.py relies on, asserted from the oracle alone (no GPU): every update of every case of
metropolis_cases.py accepts between 25 % and 90 % of its proposals with updates on both sides of the target 0.65, at most one
row per case has a decision inside the rounding band (that count is the GPU test's cap: a condition on the inputs, not a
tolerance), the float32 oracle stays inside a quarter of the tolerance of the float64 one, the special rows have the ratio sizes
they are named after, and every one-line mutant of the transition, of its rule and of the call is visible: at least 100 tolerances
away on a quarter of the chains, or another direction of a scaling, or another decision (or log-weight) of a special row."""
import numpy as np
import pytest
import torch

import metropolis_cases as mt
from helpers import close, worst, RTOL
from oracle import ais as oais

CASES = mt.all_cases()
SP = list(mt.SPECIAL_ROWS)
QUARTER = RTOL / 4


def test_shapes_cover_every_column_tile_variant_and_the_tables_are_distinct():
    assert sorted(mt.VARIANT[s[:3]] for s in mt.SHAPES) == [1, 2, 4, 5, 8]
    for D, K, nodes, B in mt.SHAPES:
        assert mt.variant_of(D * nodes) == mt.VARIANT[(D, K, nodes)]
        t = mt.inputs(D, K, nodes, B)["table"]
        assert t.dtype == torch.float32 and t.shape == (2, mt.N_UPDATES) and len(set(t.reshape(-1).tolist())) == 6
        assert abs(float(t[1, 0] / t[1, -1]) - 3.0) < 1e-5 and bool((t[1, :-1] > t[1, 1:]).all())
    assert {s[:3] for s in mt.P_TARGET_SHAPES} <= {s[:3] for s in mt.SHAPES}
    assert [mt.variant_of(w) for w in (192, 193, 256, 257, 320, 321, 512)] == [4, 4, 4, 5, 5, 8, 8]


def test_hooked_copies_equal_the_oracle_bit_for_bit():
    """TraceMetropolis / CallAIS against oracle.ais.Metropolis / AIS: result, table and log-weights, float32 and float64"""
    D, K, nodes, B = mt.SHAPES[0]
    c = mt.inputs(D, K, nodes, B)
    for dtype in (torch.float32, torch.float64):
        out, op = mt.run_oracle(c, dtype)
        nf, tgt = (c["nf64"], c["t64"]) if dtype == torch.float64 else (c["nf"], c["t32"])
        ref = oais.Metropolis(2, D, nf.log_prob, tgt.log_prob, mt.N_UPDATES, alpha=mt.ALPHA, p_target=False, dtype=dtype)
        ref.noise_scalings = c["table"].to(dtype).clone()
        want = ref.transition(mt._point3(c["start"], dtype), mt.ROW, mt.BETA, c["noise_x"].to(dtype), c["noise_u"].to(dtype))
        assert torch.equal(out.x, want.x) and torch.equal(out.log_q, want.log_q) and torch.equal(out.log_p, want.log_p)
        assert torch.equal(op.noise_scalings, ref.noise_scalings) and torch.equal(op.traces[-1][-1]["accept"], ref.last_accept)
    D, K, nodes, B = mt.CALL_SHAPES[0]
    cc = mt.call_inputs(D, K, nodes, B)
    for name, sched in mt.SCHEDULES.items():
        pt, lw, info, op, _ = mt.run_call(cc, sched, torch.float32)
        nf, tgt = cc["nf"], cc["t32"]
        ref = oais.Metropolis(mt.M_CALL, D, nf.log_prob, tgt.log_prob, mt.N_CALL, alpha=mt.ALPHA, p_target=False)
        ref.noise_scalings = cc["table"].clone()
        a = oais.AIS(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, tgt.log_prob, ref, False, mt.ALPHA, mt.M_CALL)
        a.B_space = torch.tensor(sched, dtype=torch.float64)
        wpt, wlw, winfo = a.sample_and_log_weights(cc["eps0"], cc["na"], cc["nb"])
        assert torch.equal(pt.x, wpt.x) and torch.equal(lw, wlw) and torch.equal(op.noise_scalings, ref.noise_scalings), name
        assert info == winfo and pt.x.shape[0] == cc["n_alive"]


@pytest.mark.parametrize("D,K,nodes,B,p_target", CASES)
def test_acceptance_of_every_update_and_both_sides_of_the_target(D, K, nodes, B, p_target):
    c = mt.case(D, K, nodes, B, p_target)
    for n_rows in (B, 16):
        rows = slice(0, n_rows)
        share = [float(a[rows].double().mean()) for a in c["acc64"]]
        p = c["p_accept"][n_rows]
        print(f"D={D} W={D * nodes} p_target={p_target} rows {n_rows}: accepted {[round(s, 3) for s in share]}, mean acceptance "
              f"{[round(v, 4) for v in p]}")
        assert all(0.25 <= s <= 0.90 for s in share), share
        grows = mt.directions(p, mt.TARGET)                                   # (asserts the admission margin)
        assert grows.any() and not grows.all(), f"every update on one side of the target: {p}"
        for target in (mt.TARGET_LOW, mt.TARGET_HIGH):
            assert mt.directions(p, target).all() == (target == mt.TARGET_LOW)
    # the first 16 rows as a batch of their own: what the oracle computes on that batch is the sliced statement
    _, op16 = mt.run_oracle(c, torch.float64, rows=slice(0, 16))
    assert [t["p_accept"] for t in op16.traces[-1]] == c["p_accept"][16]
    # some chain accepts update 0 and is decided again later with a quantity that a refreshed start would change
    later = c["acc64"][0] & (c["trace"][0]["log_ratio"].abs() > 100 * c["band"])
    assert bool(later.any()), "no chain accepts update 0: the never-refreshed quantity cannot show"
    all_rejected = ~c["acc64"].any(0)
    print(f"rows that reject every proposal: {int(all_rejected.sum())}")


@pytest.mark.parametrize("D,K,nodes,B,p_target", CASES)
def test_float32_oracle_stays_inside_a_quarter_of_the_tolerance(D, K, nodes, B, p_target):
    c = mt.case(D, K, nodes, B, p_target)
    differ = (c["acc64"] != c["acc32"]).any(0)
    assert c["cap"] <= 1, f"{c['cap']} rows inside the rounding band: pick another seed"
    assert not bool((differ & ~c["in_band"]).any()) and int(differ.sum()) <= c["cap"]
    same = ~differ
    for k, a, b in (("x", c["o32"].x, c["o64"].x), ("log_q", c["o32"].log_q, c["o64"].log_q), ("log_p", c["o32"].log_p, c["o64"].log_p),
                    ("log_w", c["lw32"], c["lw64"])):
        print(f"{k}: fp32 oracle {worst(a[same], b[same]):.3f} tolerance units")
        assert close(a[same], b[same], QUARTER, atol_scale=0.25), (k, worst(a[same], b[same]))
    # the float32 oracle's own table is the numpy statement (float32 * and / by 1.05), on either batch
    if not bool(differ.any()):
        assert torch.equal(c["table32"], mt.expected_table(c, B))


# name -> (class, applies to this case, condition: "quarter" / "direction" / "either")
T_MUTANTS = {
    "prev refreshed on accept": (mt.PrevRefreshed, lambda p: True, "either"),
    "no clamp in the mean": (mt.NoClampInTheMean, lambda p: True, "direction"),
    "column 0 for every update": (mt.ColumnZeroForEveryUpdate, lambda p: True, "quarter"),
    "rule inverted": (mt.RuleInverted, lambda p: True, "direction"),
    "the other target's coefficients": (mt.CoefficientsOfTheOtherTarget, lambda p: p, "quarter"),
}


@pytest.mark.parametrize("D,K,nodes,B,p_target", CASES)
def test_every_mutant_of_the_transition_is_visible(D, K, nodes, B, p_target):
    c = mt.case(D, K, nodes, B, p_target)
    want = mt.expected_table(c, B)
    for name, (cls, applies, cond) in T_MUTANTS.items():
        if not applies(p_target):
            continue
        out, op = mt.run_oracle(c, torch.float64, cls=cls)
        moved = mt.moved_rows(c, out, mt.log_w_after(c, out, c["lw_in"]))
        row = c["table"][mt.ROW - 1]
        turned = int(((op.noise_scalings[mt.ROW - 1] > row.double()) != (want[mt.ROW - 1] > row)).sum())   # the mutant's own table
        print(f"{name}: {int(moved.sum())} of {B} chains more than 100 tolerances away, {turned} directions turned")
        quarter = float(moved.double().mean()) >= 0.25
        assert {"quarter": quarter, "direction": turned > 0, "either": quarter or turned > 0}[cond], (name, int(moved.sum()), turned)
    # log_w increment from the start point's densities
    lw = mt.log_w_after(c, mt._point3(c["start"], torch.float64), c["lw_in"])
    moved = mt.moved_rows(c, c["o64"], lw)
    print(f"log_w from the start point: {int(moved.sum())} of {B} chains")
    assert float(moved.double().mean()) >= 0.25


@pytest.mark.parametrize("D,K,nodes,B,p_target", CASES)
def test_special_rows_have_their_ratio_sizes_and_the_float32_statement_rejects_them(D, K, nodes, B, p_target):
    c, s = mt.case(D, K, nodes, B, p_target), mt.special(D, K, nodes, B, p_target)
    r32, r64, rnan, rinf = SP
    lo, hi = mt.F32_WINDOW
    d32, d64 = s["ratios"][r32], s["ratios"][r64]
    print(f"log ratios: float32 row {d32.tolist()}, float64 row {d64.tolist()}")
    assert bool(((d32 >= lo) & (d32 <= hi)).all()) and bool((d64 > mt.F64_WINDOW[0]).all()) and bool(torch.isfinite(d64).all())
    for n in range(mt.N_UPDATES):
        t32, t64 = s["trace32"][n], s["trace64"][n]
        # float32: exp overflows on both tail rows -> rejected, 0 in the mean; float64 accepts the first one with ratio 1 in the mean
        assert bool(torch.isinf(torch.exp(t32["log_ratio"][[r32, r64]])).all()) and not bool(t32["accept"][SP].any())
        assert bool((t32["acc"][SP] == 0).all())
        assert bool(t64["accept"][r32]) and not bool(t64["accept"][[r64, rnan, rinf]].any())
        assert bool(torch.isnan(t32["log_ratio"][rnan])) and float(t32["log_ratio"][rinf]) == float("inf")
    st = s["start"]
    assert bool(torch.isfinite(st.log_q[[r32, r64]]).all()) and bool(torch.isfinite(st.log_p[[r32, r64]]).all())
    assert bool(torch.isnan(st.log_q[rnan])) and float(st.log_p[rinf]) == -float("inf") and bool(torch.isfinite(st.x[rinf]).all())
    keep = torch.equal(s["o32"].x[SP].nan_to_num(nan=7.0), st.x[SP].float().nan_to_num(nan=7.0))
    assert keep, "a special row moved in the float32 oracle"
    # the other rows are the plain case's, bit for bit (the rows of a transition do not interact)
    live = torch.ones(B, dtype=torch.bool)
    live[SP] = False
    assert torch.equal(s["o64"].x[live], c["o64"].x[live]) and torch.equal(s["o32"].x[live], c["o32"].x[live])
    # alone in a batch the rule sees 0; a kernel that counts an overflowing ratio as 1 sees 0.75 and turns every direction
    assert s["alone_p_accept32"] == [0.0] * mt.N_UPDATES
    mt.directions(s["p_accept32"], mt.TARGET)                                             # admission of the mixed batch
    for cls in (mt.ClampBeforeNanToNum, mt.PosinfToOne):
        out, op = mt.run_oracle(c, torch.float32, cls=cls, start=st, noise_x=s["noise_x"], rows=SP)
        assert [t["p_accept"] for t in op.traces[-1]] == [0.75] * mt.N_UPDATES and bool(op.traces[-1][0]["accept"][[0, 1, 3]].all())
        assert not torch.equal(out.x.nan_to_num(nan=7.0), st.x[SP].float().nan_to_num(nan=7.0))
    # log_w updated although beta repeats: NaN on the rows whose density is not finite, where the reference leaves log_w alone
    lw = s["lw_in"]
    bad = lw + (oais.intermediate_log_prob(st, mt.BETA, mt.ALPHA, p_target) - oais.intermediate_log_prob(st, mt.BETA, mt.ALPHA, p_target))
    assert bool(torch.isnan(bad[[rnan, rinf]]).all()) and torch.equal(mt.log_w_after(c, st, lw, beta_next=mt.BETA).nan_to_num(nan=7.0), lw.nan_to_num(nan=7.0))


CALLS = [s + (name,) for s in mt.CALL_SHAPES for name in mt.SCHEDULES]
# name -> (operator class, AIS class, condition)
C_MUTANTS = {
    "mean over B instead of the live chains": (mt.MeanOverAllocatedRows, mt.CallAIS, "direction"),
    "row 0 for every transition": (mt.RowZeroForEveryTransition, mt.CallAIS, "quarter"),
    "noise rows by the original chain number": (mt.NoiseByOriginalChainNumber, mt.CallAIS, "quarter"),
    "log_w increment from the start point": (mt.TraceMetropolis, mt.IncrementFromTheStartPoint, "quarter"),
    "prev refreshed on accept": (mt.PrevRefreshed, mt.CallAIS, "either"),
    "no clamp in the mean": (mt.NoClampInTheMean, mt.CallAIS, "direction"),
    "column 0 for every update": (mt.ColumnZeroForEveryUpdate, mt.CallAIS, "quarter"),
}


@pytest.mark.parametrize("D,K,nodes,B,schedule", CALLS)
def test_whole_call_cases_and_their_mutants(D, K, nodes, B, schedule):
    c = mt.call_case(D, K, nodes, B, schedule)
    M, nv = mt.M_CALL, c["n_alive"]
    assert c["pt64"].x.shape[0] == nv == {37: 31, 20: 15}[B] and c["pt32"].x.shape[0] == nv
    assert c["kept"].tolist() == [r for r in range(B) if r not in mt.DEAD[B]]
    assert nv % 16 != 0 and -(-nv // 16) < -(-B // 16)                       # a ragged block and an entirely dead one
    share = c["dec64"].double().mean(1)
    print(f"{schedule}: accepted per update {[round(float(s), 3) for s in share]}, mean acceptance {np.round(c['p_accept'], 4).tolist()}")
    assert bool(((share >= 0.25) & (share <= 0.90)).all())
    grows = c["p_accept"] > mt.TARGET
    assert grows.any() and not grows.all()
    assert c["cap"] <= 1
    same = (c["dec64"] == c["dec32"]).all(0)
    assert not bool((~same & ~c["in_band"]).any()) and int((~same).sum()) <= c["cap"]
    for k, a, b in (("x", c["pt32"].x, c["pt64"].x), ("log_q", c["pt32"].log_q, c["pt64"].log_q), ("log_p", c["pt32"].log_p, c["pt64"].log_p),
                    ("log_w", c["lw32"], c["lw64"])):
        print(f"{k}: fp32 oracle {worst(a[same], b[same], M * RTOL):.3f} tolerance units")
        assert close(a[same], b[same], M * RTOL, atol_scale=M), (k, worst(a[same], b[same], M * RTOL))
    if bool(same.all()):
        assert torch.equal(c["table32"], c["expected"])
    if schedule == "repeat":                                                # the transition at the repeated value leaves log_w alone
        j = [k for k in range(1, M + 1) if c["schedule"][k + 1] == c["schedule"][k]]
        assert len(j) == 1 and torch.equal(c["snapshots"][j[0]][1], c["snapshots"][j[0] - 1][1])
    base = dict(lw_in=torch.zeros(nv, dtype=torch.float64), lw64=c["lw64"], o64=c["pt64"])
    for name, (op_cls, ais_cls, cond) in C_MUTANTS.items():
        pt, lw, _, op, _ = mt.run_call(c, c["schedule"], torch.float64, op_cls, ais_cls)
        moved = mt.moved_rows(base, pt, lw)
        p = np.array([[t["p_accept"] for t in tr] for tr in op.traces])
        turned = int(((p > mt.TARGET) != grows).sum())
        print(f"{name}: {int(moved.sum())} of {nv} chains more than 100 tolerances away, {turned} directions turned")
        quarter = float(moved.double().mean()) >= 0.25
        assert {"quarter": quarter, "direction": turned > 0, "either": quarter or turned > 0}[cond], (name, int(moved.sum()), turned)
    # "log_w updated when beta repeats": the increment at a repeated value is num - den of the SAME expression, exactly zero on every
    # chain with finite densities, and the two filters leave no other chain in a call - in a call the mutant cannot show.  It shows
    # on the special rows of the teacher-forced transition (log_w turns NaN; asserted with them above and on the GPU).
    pt, lw, _, _, _ = mt.run_call(c, c["schedule"], torch.float64, ais_cls=mt.LogWMovesWhenBetaRepeats)
    assert torch.equal(lw, c["lw64"])


@pytest.mark.parametrize("n_updates", mt.NUP_COUNTS)
def test_any_number_of_updates_has_robust_directions(n_updates):
    c = mt.nup_case(n_updates)
    for p in (c["p_one"], c["p_call"]):
        assert bool((np.abs(p - mt.NUP_TARGET) >= mt.NUP_ROBUST).all()), (float(p.min()), float(p.max()))
        if n_updates > 1:
            assert (p > mt.NUP_TARGET).any() and not (p > mt.NUP_TARGET).all()
    t = c["table"]
    assert t.shape == (mt.NUP_M, n_updates)
    ratio = c["want_call"].double() / t.double()
    assert bool((((ratio - 1.05).abs() < 1e-6) | ((ratio - 1 / 1.05).abs() < 1e-6)).all())
    assert torch.equal(c["want_one"][:-1], t[:-1]) and not bool((c["want_one"][-1] == t[-1]).any())
