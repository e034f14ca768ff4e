"""The native Metropolis transition (k_metropolis<1 | 2 | 4 | 5 | 8>, metropolis_body) and its noise-scaling rule
(k_metropolis_adapt, k_metropolis_adapt_gathered) away from D = 2, against the float64 oracle (cases and their conditions:
tests/metropolis_cases.py, asserted on the CPU by tests/test_metropolis_cases.py).

ONE criterion for every comparison with the oracle: `helpers.close` at RTOL against float64 for x, log_q, log_p and log_w (a
whole call of M transitions: M x RTOL, as the other files).  A chain may take another decision than the float64 oracle only if
one of its float64 margins lies inside the rounding band of test_gpu_stressed_flow.py's transition, and on at most `cap` rows per
case (0 or 1, asserted on the CPU).  The noise scalings are compared BIT FOR BIT with the numpy float32 statement
(s * float32(1.05) or s / float32(1.05), direction from the float64 oracle's mean acceptance, which is at least 1e-3 from the
target in every admitted case).  The special rows (ratio overflowing float32 / float64, NaN coordinate, log_p = -inf) follow the
float32 statement: rejected, kept bit for bit, 0 in the mean.

Lines starting with "MEASURE" give the worst error of the HIP result and of the float32 oracle in tolerance units."""
import numpy as np
import pytest
import torch

import hmc_mass_cases as mc
import metropolis_cases as mt
from helpers import close, worst, RTOL
from oracle import numerical as onum
from test_gpu_parity import hip_flow_from_oracle, DEV

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops, parallel      # noqa: E402

CASES = mt.all_cases()
SP = list(mt.SPECIAL_ROWS)
_parts = {}


def hip_parts(c):
    """the HIP twins of the case's oracle flow and target, built once per session"""
    key = (id(c["nf"]), id(c["t64"]))
    if key not in _parts:
        D = c["D"]
        if c.get("gmm") is not None:
            locs, scales = c["gmm"]
            tg = fa.GMM(D, locs.shape[0], 1.0, true_expectation_estimation_n_samples=1000, locs=locs, scales=scales).to(DEV)
            assert torch.equal(tg.locs.cpu(), locs) and torch.equal(tg.scales.cpu(), scales)
        else:
            tg = fa.ManyWellEnergy(D)
        _parts[key] = (hip_flow_from_oracle(c["nf"]), tg)
    return _parts[key]


def make_op(c, table, target=mt.TARGET, **kw):
    hf, tg = hip_parts(c)
    op = fa.Metropolis(table.shape[0], c["D"], hf.log_prob, tg.log_prob, n_updates=table.shape[1], alpha=mt.ALPHA,
                       p_target=c["p_target"], target_p_accept=target, **kw).to(DEV)
    assert op.is_native and op.noise_scalings.shape == table.shape
    op.noise_scalings.copy_(table)
    return op


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(bits(a), bits(b))


def run_transition(c, op, rows=slice(None), start=None, noise_x=None, lw_in=None, beta_next=mt.BETA_NEXT, with_log_w=True,
                   i=mt.ROW, noise_u=None):
    """one teacher-forced transition on rows `rows` of the case's (or the given) start: (Point, log_w, the float32 inputs), CPU"""
    s = c["start"] if start is None else start
    pt = fa.Point(*(t[rows].float().to(DEV).contiguous() for t in (s.x, s.log_q, s.log_p)))
    given = fa.Point(pt.x.cpu().clone(), pt.log_q.cpu().clone(), pt.log_p.cpu().clone())
    lw0 = (c["lw_in"] if lw_in is None else lw_in)[rows].float()
    lw = lw0.to(DEV) if with_log_w else None
    nx = (c["noise_x"] if noise_x is None else noise_x)[:, rows].contiguous().to(DEV)
    nu = (c["noise_u"] if noise_u is None else noise_u)[:, rows].contiguous().to(DEV)
    op.transition(pt, i, mt.BETA, log_w=lw, beta_next=beta_next, noise_x=nx, noise_u=nu)
    torch.cuda.synchronize()
    return fa.Point(pt.x.cpu(), pt.log_q.cpu(), pt.log_p.cpu()), (lw.cpu() if with_log_w else None), given, lw0


def check(tag, c, out, lw, rows=slice(None), live=None):
    """the one criterion against the float64 oracle of case `c` on its rows `rows` (`live`: the rows of the batch to compare).
    Returns the rows whose decision differs."""
    o64, o32 = c["o64"], c["o32"]
    live = torch.ones(out.x.shape[0], dtype=torch.bool) if live is None else live
    differ = (mc.tol_units(out.x, o64.x[rows]) > 1) & live                # a chain that took another decision sits at another candidate
    outside = differ & ~c["in_band"][rows]
    assert not bool(outside.any()), f"{tag}: rows {outside.nonzero().flatten().tolist()} differ from float64 outside the rounding band"
    assert int(differ.sum()) <= c["cap"], f"{tag}: {int(differ.sum())} decisions differ, the case has {c['cap']} rows inside the band"
    same = live & ~differ
    same32 = same & (c["acc32"] == c["acc64"]).all(0)[rows]
    q = [("x", out.x, o32.x[rows], o64.x[rows]), ("log_q", out.log_q, o32.log_q[rows], o64.log_q[rows]),
         ("log_p", out.log_p, o32.log_p[rows], o64.log_p[rows])]
    if lw is not None:
        q.append(("log_w", lw, c["lw32"][rows], c["lw64"][rows]))
    for k, a, b32, b64 in q:
        print(f"MEASURE {tag} | {k} | HIP {worst(a[same], b64[same]):.2f} | fp32 oracle {worst(b32[same32], b64[same32]):.2f}")
    for k, a, b32, b64 in q:
        assert close(a[same], b64[same]), f"{tag}: {k} is {worst(a[same], b64[same]):.2f} tolerances from float64"
    return differ


def assert_variant(c):
    """the column-tile variant the dispatcher takes for this width (train_step_plan reports padded width / 64 of the same FlowDims)"""
    D, K, W = c["D"], c["K"], c["D"] * c["nodes"]
    assert int(_ops.load().train_step_plan(D, K, W)[1]) == mt.VARIANT[(D, K, c["nodes"])] == mt.variant_of(W)


# ---- (a) one teacher-forced transition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", ["all", 16])
@pytest.mark.parametrize("D,K,nodes,B,p_target", CASES)
def test_single_transition_on_every_column_tile_variant(D, K, nodes, B, p_target, n_rows):
    c = mt.case(D, K, nodes, B, p_target)
    n_rows = B if n_rows == "all" else n_rows
    rows = slice(0, n_rows)
    assert_variant(c)
    op = make_op(c, c["table"])
    out, lw, given, _ = run_transition(c, op, rows)
    tag = f"a D={D} W={D * nodes} variant {mt.VARIANT[(D, K, nodes)]} p_target={p_target} rows {n_rows}"
    differ = check(tag, c, out, lw, rows)
    got, want = op.noise_scalings.cpu(), mt.expected_table(c, n_rows)
    assert same_bits(got[:mt.ROW - 1], c["table"][:mt.ROW - 1]), "a row of another transition changed"
    if not bool(differ.any()):
        assert same_bits(got, want), f"{tag}: scalings {got[mt.ROW - 1].tolist()} != the statement {want[mt.ROW - 1].tolist()}"
    # rows that rejected all three proposals are not written
    rejected = ~c["acc64"].any(0)[rows] & ~differ
    for a, b in ((out.x, given.x), (out.log_q, given.log_q), (out.log_p, given.log_p)):
        assert same_bits(a[rejected], b[rejected])
    moved = (out.x != given.x).any(1)
    assert torch.equal(moved[~differ], c["acc64"].any(0)[rows][~differ])


# ---- (b) rule switches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [mt.TARGET_LOW, mt.TARGET_HIGH], ids=["grow", "shrink"])
@pytest.mark.parametrize("D,K,nodes,B", mt.SHAPES)
def test_rule_with_the_target_below_and_above_every_mean_acceptance(D, K, nodes, B, target):
    c = mt.case(D, K, nodes, B)
    op = make_op(c, c["table"], target=target)
    run_transition(c, op)
    assert same_bits(op.noise_scalings.cpu(), mt.expected_table(c, B, target))
    grew = op.noise_scalings.cpu()[mt.ROW - 1] > c["table"][mt.ROW - 1]
    assert bool(grew.all()) == (target == mt.TARGET_LOW) and bool((~grew).all()) == (target == mt.TARGET_HIGH)


@pytest.mark.parametrize("D,K,nodes,B", [mt.SHAPES[3], mt.SHAPES[4]])
def test_rule_switched_off_leaves_the_table_alone_and_the_point_is_the_tuned_run_s(D, K, nodes, B):
    c = mt.case(D, K, nodes, B)
    out, lw, _, _ = run_transition(c, make_op(c, c["table"]))
    for kw in (dict(adjust_step_size=False), dict(eval_mode=True), dict(adjust_step_size=False, eval_mode=True)):
        op = make_op(c, c["table"], **kw)
        o2, lw2, _, _ = run_transition(c, op)
        assert same_bits(op.noise_scalings.cpu(), c["table"]), kw
        assert same_bits(o2.x, out.x) and same_bits(o2.log_q, out.log_q) and same_bits(o2.log_p, out.log_p) and same_bits(lw2, lw)
    # log_w = None is accepted; the point and the table are the same
    op = make_op(c, c["table"])
    o3, lw3, _, _ = run_transition(c, op, with_log_w=False)
    assert lw3 is None and same_bits(o3.x, out.x) and same_bits(o3.log_p, out.log_p)
    assert same_bits(op.noise_scalings.cpu(), mt.expected_table(c, B))


@pytest.mark.parametrize("D,K,nodes,B", [mt.SHAPES[0], mt.SHAPES[4]])
def test_a_repeated_beta_leaves_log_w_bit_unchanged(D, K, nodes, B):
    """ais.py:93 - also on the rows whose densities are not finite, where num - den of the same expression is NaN"""
    c, s = mt.case(D, K, nodes, B), mt.special(D, K, nodes, B)
    out, lw, _, _ = run_transition(c, make_op(c, c["table"]), start=s["start"], noise_x=s["noise_x"], lw_in=s["lw_in"])
    o2, lw2, _, lw0 = run_transition(c, make_op(c, c["table"]), start=s["start"], noise_x=s["noise_x"], lw_in=s["lw_in"],
                                     beta_next=mt.BETA)
    assert same_bits(lw2, lw0) and same_bits(o2.x, out.x)
    assert not same_bits(lw, lw0)


# ---- (c) special rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K,nodes,B,p_target", CASES)
def test_special_rows_are_rejected_and_add_nothing_to_the_mean(D, K, nodes, B, p_target):
    c, s = mt.case(D, K, nodes, B, p_target), mt.special(D, K, nodes, B, p_target)
    tag = f"c D={D} W={D * nodes} p_target={p_target}"
    # among live rows
    op = make_op(c, c["table"])
    out, lw, given, _ = run_transition(c, op, start=s["start"], noise_x=s["noise_x"], lw_in=s["lw_in"])
    for a, b in ((out.x, given.x), (out.log_q, given.log_q), (out.log_p, given.log_p)):
        assert same_bits(a[SP], b[SP]), f"{tag}: a special row was written"
    print(f"MEASURE {tag} | device exp() of the log ratios {[round(float(v), 1) for v in s['ratios'][SP[0]]]} (float32 row) and "
          f"{[round(float(v), 1) for v in s['ratios'][SP[1]]]} (float64 row) | rejected: not finite, as the reference's float32 exp")
    live = torch.ones(B, dtype=torch.bool)
    live[SP] = False
    differ = check(tag + " live rows", c, out, lw, live=live)
    # the live rows do not see their neighbours: bit for bit the plain batch's
    plain, plw, _, _ = run_transition(c, make_op(c, c["table"]))
    assert same_bits(out.x[live], plain.x[live]) and same_bits(out.log_q[live], plain.log_q[live]) and same_bits(lw[live], plw[live])
    if not bool(differ.any()):
        want = c["table"].numpy().copy()
        want[mt.ROW - 1] = mt.rule_statement(want[mt.ROW - 1], mt.directions(s["p_accept32"], mt.TARGET))
        assert same_bits(op.noise_scalings.cpu(), torch.from_numpy(want)), f"{tag}: the rule saw another mean than the float32 statement"
    # alone in a batch: the mean is 0 - every scaling shrinks; a kernel that counted an overflowing ratio as 1 would see 0.75 > 0.65
    op = make_op(c, c["table"])
    out, lw, given, _ = run_transition(c, op, rows=SP, start=s["start"], noise_x=s["noise_x"], lw_in=s["lw_in"])
    for a, b in ((out.x, given.x), (out.log_q, given.log_q), (out.log_p, given.log_p)):
        assert same_bits(a, b), f"{tag}: a special row alone in its batch was written"
    want = c["table"].numpy().copy()
    want[mt.ROW - 1] = mt.rule_statement(want[mt.ROW - 1], [False] * mt.N_UPDATES)
    assert same_bits(op.noise_scalings.cpu(), torch.from_numpy(want))


# ---- (d) whole calls ------------------------------------------------------------------------------------------------------------
M = mt.M_CALL
CALLS = [s + (name,) for s in mt.CALL_SHAPES for name in mt.SCHEDULES]


def call_sampler(c, table, schedule, tau=None, target=mt.TARGET):
    hf, tg = hip_parts(c)
    op = make_op(c, table, target=target)
    ais = fa.AnnealedImportanceSampler(hf, tg.log_prob, op, False, mt.ALPHA, table.shape[0], distribution_spacing_type=list(schedule),
                                       resample_threshold=tau)
    assert ais.is_native and ais.B_space.tolist() == list(schedule)
    return op, ais


def check_call(tag, c, pt, lw, info):
    FR = M * RTOL
    p64, p32 = c["pt64"], c["pt32"]
    x = pt.x.cpu()
    assert x.shape[0] == c["n_alive"], f"{tag}: {x.shape[0]} survivors, the oracle has {c['n_alive']}"
    scale = max(1.0, float(p64.x.abs().max()))
    moved = ((x.double() - p64.x).abs() > FR * p64.x.abs() + 2e-6 * M * scale).any(1)
    print(f"MEASURE {tag} | chains that left the oracle | {moved.nonzero().flatten().tolist()} | inside the band "
          f"{c['in_band'].nonzero().flatten().tolist()}")
    assert not bool((moved & ~c["in_band"]).any()) and int(moved.sum()) <= c["cap"], f"{tag}: rows {moved.nonzero().flatten().tolist()}"
    ok = ~moved
    ok32 = ok & (c["dec32"] == c["dec64"]).all(0)
    for k, a, b32, b64 in (("x", x, p32.x, p64.x), ("log_q", pt.log_q.cpu(), p32.log_q, p64.log_q),
                           ("log_p", pt.log_p.cpu(), p32.log_p, p64.log_p), ("log_w", lw.cpu(), c["lw32"], c["lw64"])):
        print(f"MEASURE {tag} | {k} | HIP {worst(a[ok], b64[ok], FR):.2f} | fp32 oracle {worst(b32[ok32], b64[ok32], FR):.2f}")
        assert close(a[ok], b64[ok], FR, atol_scale=M), f"{tag}: {k} is {worst(a[ok], b64[ok], FR):.2f} tolerances from float64"
    # the statistics: the float64 formulas on the call's own log-weights, and (no chain having left) the float64 oracle's
    lwd = lw.cpu().double()
    own = (float(onum.effective_sample_size(lwd)), float(torch.logsumexp(lwd, 0) - np.log(c["B"])))
    got = (info.ess_ais, info.log_Z)
    print(f"MEASURE {tag} | ess_ais, log_Z | HIP {got} | float64 on its log_w {own} | oracle {c['info64']}")
    for g, w in zip(got, own):
        assert close(np.float64(g), np.float64(w), FR), (g, w)
    if not bool(moved.any()):
        for g, w in zip((info.ess_base,) + got, c["info64"]):
            assert close(np.float64(g), np.float64(w), FR, atol_scale=M), (tag, g, w)
    return moved


def fused(c, schedule, **kw):
    op, ais = call_sampler(c, c["table"], schedule, **kw)
    extra = {} if kw.get("tau") is None else dict(noise_r=torch.full((M,), 0.37, dtype=torch.float64, device=DEV))
    pt, lw = ais.sample_and_log_weights(c["B"], eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV), **extra)
    return op, ais, pt, lw


@pytest.mark.parametrize("D,K,nodes,B,schedule", CALLS)
def test_whole_call_with_dying_chains_and_its_other_entries(D, K, nodes, B, schedule):
    c = mt.call_case(D, K, nodes, B, schedule)
    tag = f"d D={D} W={D * nodes} {schedule}"
    op, ais, pt, lw = fused(c, c["schedule"])
    moved = check_call(tag, c, pt, lw, ais._logging_info)
    table = op.noise_scalings.cpu()
    if not bool(moved.any()):
        assert same_bits(table, c["expected"]), f"{tag}: {table.tolist()} != the statement {c['expected'].tolist()}"
    assert not bool((table == c["table"]).any())                                  # every entry moved by one factor
    # the same call in pieces through ais_phase: chain initialisation | transitions 1, 2 | transition 3 and the end
    op2, ais2 = call_sampler(c, c["table"], c["schedule"])
    st = ais2.new_phase_state(B, c["eps0"].to(DEV), c["na"].to(DEV), c["nb"].to(DEV))
    ais2.enqueue_phase(st, 1, 1, 0)
    ais2.enqueue_phase(st, 0, 1, 2)
    ais2.enqueue_phase(st, 2, 3, M)
    nv = c["n_alive"]
    assert int(st["n_valid"][0]) == nv and int(st["n_valid"][1]) == nv
    for a, b in ((st["x"][:nv], pt.x), (st["lq"][:nv], pt.log_q), (st["lp"][:nv], pt.log_p), (st["log_w"][:nv], lw),
                 (op2.noise_scalings, op.noise_scalings)):
        assert same_bits(a, b), f"{tag}: the call in pieces differs"
    # SMC mode, threshold 0: the decision runs in front of every transition and never resamples
    op3, ais3, pt3, lw3 = fused(c, c["schedule"], tau=0.0)
    assert int(ais3.last_smc[0].sum()) == 0
    for a, b in ((pt3.x, pt.x), (pt3.log_q, pt.log_q), (pt3.log_p, pt.log_p), (lw3, lw), (op3.noise_scalings, op.noise_scalings)):
        assert same_bits(a, b), f"{tag}: SMC mode without a resampling differs"
    # the rule deferred to the end of the call, on one rank (k_metropolis_adapt_gathered on the call's own slab)
    op4, ais4 = call_sampler(c, c["table"], c["schedule"])
    be = parallel.HipShardBackend(ais4)
    pt4, lw4, slab = be.run_metropolis_deferred(B, c["eps0"].to(DEV), c["na"].to(DEV), c["nb"].to(DEV))
    assert same_bits(op4.noise_scalings.cpu(), c["table"])
    be.adapt_metropolis(slab, 1, B)
    for a, b in ((pt4.x, pt.x), (pt4.log_q, pt.log_q), (lw4, lw), (op4.noise_scalings, op.noise_scalings)):
        assert same_bits(a, b), f"{tag}: the deferred rule differs"


# ---- (e) any number of updates --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_updates", mt.NUP_COUNTS)
def test_every_update_s_scaling_is_adapted_whatever_their_number(n_updates):
    """the reference has no bound on n_updates: through `transition` and through the whole call every column of the table moves
    by exactly one factor, in the statement's direction (the rule kernel strides over the updates)"""
    c = mt.nup_case(n_updates)
    B = c["B"]
    op = make_op(c, c["table"], target=mt.NUP_TARGET)
    run_transition(c, op, start=c["start"], noise_x=c["na"][-1], noise_u=c["nb"][-1], lw_in=torch.zeros(B), i=mt.NUP_M)
    got = op.noise_scalings.cpu()
    untouched = (got[-1] == c["table"][-1]).nonzero().flatten().tolist()
    assert not untouched, f"transition: columns {untouched[:4]} .. of {n_updates} were never adapted"
    assert same_bits(got, c["want_one"])
    op2, ais = call_sampler(c, c["table"], c["schedule"], target=mt.NUP_TARGET)
    pt, lw = ais.sample_and_log_weights(B, eps0=c["eps0"].to(DEV), noise_a=c["na"].to(DEV), noise_b=c["nb"].to(DEV))
    assert pt.x.shape[0] == B and bool(torch.isfinite(lw).all())
    got = op2.noise_scalings.cpu()
    untouched = (got == c["table"]).any(0).nonzero().flatten().tolist()
    assert not untouched, f"whole call: columns {untouched[:4]} .. of {n_updates} were never adapted"
    assert same_bits(got, c["want_call"])
