"""CPU tests of the case list of the fixed-point resamplers (tests/resample_fixed_cases.py): every device branch the list is
there for is reached - judged by `branch_profile`, which sees the oracle's output alone - and the oracle agrees with itself
on every case.  A later edit of a case, or of a kernel constant mirrored in the case module, that stops a branch being
reached fails here, without a GPU."""
import functools

import numpy as np
import pytest

import resample_fixed_cases as rc
from oracle import numerical as onum


@functools.lru_cache(maxsize=None)
def _profiles():
    """(case name, ns, profile) of every case of the list at u0 = 0.37 (the branch a wave takes does not hinge on u0: it moves
    every run by less than one stratum; the claims below keep away from the thresholds by more than that)."""
    out = []
    for name in rc.ALL_NAMES:
        case = rc.get_case(name)
        for ns in case.ns:
            out.append((name, ns, rc.branch_profile(case.log_w, ns, 0.37)))
    return out


def _where(pred):
    return [(name, ns) for name, ns, p in _profiles() if pred(p)]


def test_constants_and_capacity_formula():
    assert rc.EM_WIN < rc.EM_GIANT < rc.EM_F64_STRATA and rc.SCAN_TILE == rc.SYS_CHUNK == 4 * rc.EM_WAVE_ITEMS
    # (70001 - (69 + 2 * 18 + 5)) / 3 = 23297, capped by ns / EM_GIANT + 1
    assert rc.giant_capacity(70_001, 70_001) == 3 and rc.giant_capacity(70_001, (1 << 21) + 3) == 65
    assert rc.giant_capacity(12, 480_000) == 1 and rc.giant_capacity(5, 200_000) == 0 and rc.giant_capacity(1, 10) == 0
    assert rc.giant_capacity(300, (1 << 20) + 5) == 33
    for name in rc.ALL_NAMES:
        case = rc.get_case(name)
        assert case.log_w.dtype == np.float32 and len(case.log_w) <= 70_001 and max(case.ns) <= 2_100_000 and min(case.ns) >= 1
        if name in rc.SPECIAL_NAMES and len(case.log_w) > 300:
            assert len(case.log_w) == rc.SPECIAL_N


def test_several_windows_without_the_giant_branch():
    """EM_WIN < T < EM_GIANT: more than one marker window, `T >= EM_GIANT` false."""
    hit = _where(lambda p: bool(((p["strata"] > rc.EM_WIN) & (p["strata"] < rc.EM_GIANT) & (p["giants"] == 0)).any()))
    assert hit, "no case has a wave of several windows below the giant threshold"
    assert any(name.startswith("edge_") for name, _ in hit)


def test_giant_branch_entered_without_a_giant_run():
    """hot_wave at ns = n: the wave owns >= EM_GIANT strata, looks for giant runs and finds none."""
    hit = _where(lambda p: bool(((p["strata"] >= rc.EM_GIANT) & (p["giants"] == 0)).any()))
    assert ("hot_wave", rc.SPECIAL_N) in hit


def test_published_giant_beside_ordinary_runs_in_one_wave():
    hit = _where(lambda p: bool(((p["giants"] >= 1) & (p["distinct"] >= p["giants"] + 100)).any())
                 and p["giants"].sum() <= p["capacity"])
    assert any(name == "mixed" for name, _ in hit), hit


def test_float64_estimate_twice_once_with_real_work():
    big = _where(lambda p: bool((p["strata"] >= rc.EM_F64_STRATA).any()))
    assert len({name for name, _ in big}) >= 2, big
    work = _where(lambda p: bool(((p["strata"] >= rc.EM_F64_STRATA) & (p["distinct"] >= 100)).any()))
    assert work, "no wave with T >= 2^20 and at least 100 distinct indices"
    assert ("few_weights_many_draws", (1 << 20) + 5) in big      # a ragged last wave (300 weights) that owns everything


def test_giant_list_full_and_absent():
    full = _where(lambda p: p["capacity"] >= 1 and p["giants"].sum() > p["capacity"])
    assert ("list_full", 480_000) in full
    none = _where(lambda p: p["capacity"] == 0 and p["giants"].sum() >= 1)
    assert ("no_list", 200_000) in none


def test_a_chunk_spans_more_tiles_than_are_staged():
    hit = _where(lambda p: p["chunk_span"] > rc.SYS_MAX_SPAN)
    assert {"heavy_tail", "dead_middle"} <= {name for name, _ in hit}, hit
    assert _where(lambda p: 1 < p["chunk_span"] <= rc.SYS_MAX_SPAN)        # and the staged path walks several tiles


def test_all_dead_has_total_zero_and_only_all_dead():
    dead = {name for name, _, p in _profiles() if p["total"] == 0}
    assert dead == {"all_dead"}
    case = rc.get_case("all_dead")
    assert (rc.expected_systematic(case, 77, 0.37) == rc.SPECIAL_N - 1).all()
    assert (rc.expected_multinomial(case, np.array([0.0, 0.5])) == rc.SPECIAL_N - 1).all()


def test_u0_edges_are_edges():
    """u0 = 0 gives U = 0 and the float64 below 1 gives U = S - 1 or the float64 product below it: the ends of the offset."""
    for name in ("edge_17", "heavy_tail", "all_equal"):
        case = rc.get_case(name)
        for ns in case.ns:
            _, S, U = onum.systematic_strata(rc.total_of(case), ns, rc.U0[1])
            assert U == 0
            _, S, U = onum.systematic_strata(rc.total_of(case), ns, rc.U0[2])
            assert S - 1 - U <= S >> 52


@pytest.mark.parametrize("name", ["mixed", "unaligned", "hot_wave"])
def test_constructed_u0_puts_a_threshold_on_a_step_where_the_estimate_is_one_high(name):
    """The fourth u0 of these cases: some stratum's threshold equals a CDF value exactly (K(C) is an exact quotient) and the
    float64 estimate of `stratum_rel` exceeds it, so only the `--k` branch of its correction step gives the oracle's index -
    at a wave's first stratum (d = 0: K0 and the previous wave's T) and, for hot_wave, at an item of a wave with T >= 2^20."""
    case = rc.get_case(name)
    assert len(case.u0) == 4 and case.on_step is not None, "no overshooting on-step u0 found for this case any more"
    ns, c0, d = case.on_step
    u0, total = case.u0[3], rc.total_of(case)
    assert ns in case.ns and 0.0 <= u0 < 1.0
    F, S, U = onum.systematic_strata(total, ns, u0)
    assert (((c0 + d) << F) - U) % S == 0
    m = (((c0 + d) << F) - U) // S
    assert 0 < m < ns and (m * S + U) >> F == c0 + d
    est, exact = rc.f64_estimate(total, ns, u0, c0, d)
    assert exact == m and est == m + 1
    C = rc.expected_cdf(case)
    j = int(np.searchsorted(C, c0 + d, side="left"))
    assert int(C[j]) == c0 + d
    idx = rc.expected_systematic(case, ns, u0)
    assert idx[m - 1] <= j < idx[m]                       # stratum m is the first one beyond item j
    if name == "hot_wave":
        assert d > 0 and 2048 <= j < 3072
        assert rc.branch_profile(case.log_w, ns, u0)["strata"][2] >= rc.EM_F64_STRATA
    else:
        assert d == 0 and (j + 1) % rc.EM_WAVE_ITEMS == 0


@pytest.mark.parametrize("name", rc.ALL_NAMES)
def test_oracle_agrees_with_itself(name):
    """systematic_fixed: non-decreasing, in [0, n), every count within 1 of ns W / total (the truncation of the stratum width S
    to 2^-F moves a count by less than ns^2 2^-61: the 1e-6); multinomial_fixed of sorted u: non-decreasing; the thresholds of
    `multinomial_u` land on both sides of CDF steps."""
    case = rc.get_case(name)
    n = len(case.log_w)
    q = onum.fixed_point_weights(case.log_w).astype(np.float64)
    total = rc.total_of(case)
    for ns in case.ns:
        for u0 in case.u0:
            idx = rc.expected_systematic(case, ns, u0)
            assert idx.shape == (ns,) and idx.dtype == np.int64
            assert idx.min() >= 0 and idx.max() < n and np.all(np.diff(idx) >= 0)
            if total > 0:
                counts = np.bincount(idx, minlength=n)
                assert np.abs(counts - ns * q / total).max() <= 1 + 1e-6
        u = rc.multinomial_u(case, ns)
        assert u.shape == (ns,) and u.min() >= 0.0 and u.max() < 1.0
        m = rc.expected_multinomial(case, np.sort(u))
        assert m.min() >= 0 and m.max() < n and np.all(np.diff(m) >= 0)
        if total > 0:
            assert np.all(q[rc.expected_multinomial(case, u)] > 0)       # a dead weight is never drawn
    if total > 0 and max(case.ns) >= 66:
        ns = max(case.ns)
        C = rc.expected_cdf(case)
        t = np.floor(rc.multinomial_u(case, ns)[2:66] * np.float64(total)).astype(np.uint64)
        on_step = np.isin(t, C).sum()
        below_step = np.isin(t + np.uint64(1), C).sum()
        need = 8 if n >= rc.SCAN_TILE else 1
        assert on_step >= need and below_step >= need, (on_step, below_step)
