"""CPU: every claim of tests/tail_cases.py, from its two restatements, float64 torch and the oracle alone - which branch of the
reduction each weight vector reaches, that the restated reduction is the float64 statement at the suite's tolerances, what the
special values give, that every dead-row pattern has its stated survivors and every kind of death, that the restated
compaction is `field[mask]`, and that one-line mutants of either restatement are seen by a listed case."""
import functools
import math

import numpy as np
import pytest
import torch

import tail_cases as tc
from helpers import seeded_oracle_flow  # noqa: F401  (path set-up)
from oracle import ais as oais, targets as otgt

CASES = tc.weight_cases()
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def evaluated(name):
    """(restatement, float64 statement, float32 formula) of one weight case, computed once"""
    c = BY_NAME[name]
    buf = tc.buffer_of(c)
    vals = buf[c.offset:c.offset + tc.n_used(c)]
    r = tc.reduce_restated(buf, c.n_cap, c.n, tc.n_norm_of(c), c.offset)
    return r, tc.reference64(vals, tc.n_norm_of(c)), tc.reference32(vals, tc.n_norm_of(c))


def test_the_list_holds_every_size_and_family_it_states():
    assert len(BY_NAME) == len(CASES)
    sizes = {tc.n_used(c) for c in CASES if c.n is None}
    assert set(tc.EDGE_N) | {1 << 20, (1 << 20) + 1, (1 << 22) - 1, 1 << 22, (1 << 22) + 4099, (1 << 23) + 5} <= sizes
    for n in (1 << 22, (1 << 22) + 4099, (1 << 23) + 5):        # each chunk-path size also one float off alignment
        assert {c.offset for c in CASES if c.n is None and c.n_cap == n and c.family in ("chunk path", "unaligned")} == {0, 1}
    assert {c.n for c in CASES if c.family == "n_ptr"} == set(tc.N_PTRS)
    assert {c.n_cap for c in CASES if c.family == "n_ptr"} == {(1 << 22) + 4099}
    assert {c.n_norm for c in CASES} == {None, 1.0, "3n"}
    # the threshold of the float4 path: n >= 16 * stride first holds at 2^22
    assert tc.chunk_span(tc.CHUNK_FIRST_N) == tc.CHUNK_FIRST_N and tc.chunk_span(tc.CHUNK_FIRST_N - 1) > tc.CHUNK_FIRST_N - 1
    assert all(tc.chunk_span(n) > n for n in (1, 1024, 2048, 2049, 1 << 20, 1 << 21))


def test_every_branch_of_the_reduction_is_taken_by_the_case_listed_for_it():
    total = sum((evaluated(c.name)[0].counts for c in CASES), start=tc.Counter())
    for branch in ("scalar", "chunk", "push_le", "push_gt", "push_gt_late", "push_ninf", "push_nan", "push_pinf", "chunk_le",
                   "chunk_gt", "chunk_gt_late", "chunk_gt_from_ninf_late", "chunk_empty", "chunk_nan", "chunk_pinf", "merge",
                   "merge_ninf", "merge_pinf", "merge_nan"):
        assert total[branch] > 0, branch
    for c in CASES:
        k = evaluated(c.name)[0].counts
        # every element in front of the count is pushed once, nothing beyond it
        assert k["scalar"] + tc.CHUNK * k["chunk"] == tc.n_used(c), c.name
        # the float4 path runs on exactly the aligned cases of n >= 2^22
        assert (k["chunk"] > 0) == c.chunk == (c.offset == 0 and tc.n_used(c) >= tc.CHUNK_FIRST_N), c.name
    cnt = lambda name: evaluated(name)[0].counts                                                      # noqa: E731
    stride = tc.ESS_MAX_BLOCKS * tc.ESS_THREADS
    assert cnt("ascending")["push_le"] == 0 and cnt("ascending")["push_gt_late"] > 0
    assert cnt("descending")["push_gt_late"] == 0 and cnt("descending")["push_le"] > 0
    assert cnt("ascending_2^20")["push_le"] == 0 and cnt("ascending_2^20")["push_gt_late"] == 3 * stride
    assert cnt("randn_2^22")["scalar"] == 0 and cnt("randn_2^22")["chunk"] == stride
    assert cnt("randn_2^22+4099")["scalar"] == 4099 and cnt("randn_2^22_unaligned")["scalar"] == 1 << 22
    assert cnt("randn_2^23+5")["chunk"] == 2 * stride and cnt("randn_2^23+5")["scalar"] == 5
    assert cnt("randn_2^23+5")["chunk_le"] > 0 and cnt("randn_2^23+5")["chunk_gt_late"] > 0
    assert cnt("ascending_2^23+5")["chunk_gt_late"] == stride and cnt("ascending_2^23+5")["chunk_le"] == 0
    assert cnt("descending_2^23+5")["chunk_le"] == stride and cnt("descending_2^23+5")["chunk_gt_late"] == 0
    assert cnt("randn_2^22-1")["scalar"] == (1 << 22) - 1
    assert cnt("ninf_whole_chunks")["chunk_empty"] == 4 and cnt("ninf_16_blocks")["chunk_empty"] == 0
    assert cnt("ninf_first_span")["chunk_empty"] == stride and cnt("ninf_first_span")["chunk_gt_from_ninf_late"] == stride
    assert cnt("ninf_all")["merge_ninf"] > 0 and cnt("ninf_all")["push_ninf"] == 2049
    assert cnt("nan_in_chunk")["chunk_nan"] == 1 and cnt("pinf_in_chunk")["chunk_pinf"] == 1
    assert cnt("nan_in_remainder")["chunk_nan"] == 0 and cnt("nan_in_remainder")["push_nan"] == 1
    assert cnt("pinf_in_remainder")["chunk_pinf"] == 0 and cnt("pinf_in_remainder")["push_pinf"] == 1
    assert cnt("pinf_one")["merge_pinf"] > 0 and cnt("nan_one")["merge_nan"] > 0
    assert cnt("n_ptr_4194304")["scalar"] == 0 and cnt("n_ptr_4194305")["scalar"] == 1 and cnt("n_ptr_1025")["chunk"] == 0


def test_the_restated_reduction_is_the_float64_statement_at_the_suite_tolerances():
    """ESS relative 1e-5, log Z 1e-5 |log Z| + 1e-5 (test_ess_logz_vs_golden's) on every case.  The reference's own float32
    formula is printed beside it and asserted nowhere: it leaves the tolerance on long vectors."""
    worst = {}
    for c in CASES:
        r, ref64, ref32 = evaluated(c.name)
        u, u32 = tc.tol_units((r.ess, r.log_z), ref64), tc.tol_units(ref32, ref64)
        print(f"{c.name:28s} restated {u[0]:9.2e} {u[1]:9.2e}   float32 formula {u32[0]:9.2e} {u32[1]:9.2e}")
        assert max(u) <= 1.0, (c.name, u, (r.ess, r.log_z), ref64)
        assert r.n == tc.n_used(c)
        worst[c.family] = max(worst.get(c.family, 0.0), *u)
    print({k: f"{v:.2e}" for k, v in worst.items()})


def test_special_values_from_float64_torch_alone():
    t = lambda v: torch.tensor(v, dtype=torch.float64)                                                # noqa: E731
    ess, lz = oais.effective_sample_size, lambda v: torch.logsumexp(v, 0)                              # noqa: E731
    inf = math.inf
    assert math.isnan(ess(t([0.0, math.nan, 1.0]))) and math.isnan(lz(t([0.0, math.nan, 1.0])))
    assert math.isnan(ess(t([0.0, inf, 1.0]))) and lz(t([0.0, inf, 1.0])) == inf        # softmax NaN, logsumexp +inf
    assert math.isnan(ess(t([-inf, -inf]))) and lz(t([-inf, -inf])) == -inf
    assert ess(t([-7.5])) == 1.0 and lz(t([-7.5])) == -7.5
    assert ess(t([1.0, -inf, 1.0, -inf])) == 0.5                                          # -inf weighs 0 and counts in n
    for name, want in (("nan_one", (math.nan, math.nan)), ("pinf_one", (math.nan, inf)), ("ninf_all", (math.nan, -inf)),
                       ("nan_in_chunk", (math.nan, math.nan)), ("pinf_in_chunk", (math.nan, inf)),
                       ("nan_in_remainder", (math.nan, math.nan)), ("pinf_in_remainder", (math.nan, inf)), ("n_1", (1.0, -7.5))):
        r, ref64, _ = evaluated(name)
        for got in ((r.ess, r.log_z), ref64):
            assert tc.tol_units(got, want) == (0.0, 0.0), (name, got, want)
    # closed forms
    assert evaluated("constant")[0].ess == 1.0
    assert evaluated("one_dominant")[0].ess == float(np.float32(1.0 / 1025))
    assert evaluated("ninf_all_but_one")[0].ess == float(np.float32(1.0 / 2049))
    assert evaluated("pair_+-3e38_n2")[0].ess == 0.5 and evaluated("pair_+-3e38")[0].ess == float(np.float32(1.0 / 257))
    # the bait beyond n_ptr (finite, NaN, +inf) is there, and would be seen
    for k in tc.N_PTRS:
        buf = tc.buffer_of(BY_NAME[f"n_ptr_{k}"])
        assert np.isnan(buf[k:]).any() and np.isposinf(buf[k:]).any() and np.isfinite(buf[k:]).sum() > 1
        assert np.isfinite(buf[:k]).all()


# (mutant, the case that sees it)
REDUCTION_MUTANTS = (("push_s2_r", "ascending_2^20"), ("chunk_s2_r", "randn_2^23+5"), ("merge_no_rescale", "randn_2049"),
                     ("chunk_keep_m", "ascending_2^23+5"), ("ninf_not_counted", "ninf_few"), ("ess_over_cap", "n_ptr_1025"),
                     ("log_n", "n_norm_1_1025"), ("read_bait", "n_ptr_4194305"))


@pytest.mark.parametrize("mut,name", REDUCTION_MUTANTS)
def test_one_line_mutants_of_the_restated_reduction_are_100_tolerances_away(mut, name):
    c = BY_NAME[name]
    good = evaluated(name)[0]
    bad = tc.reduce_restated(tc.buffer_of(c), c.n_cap, c.n, tc.n_norm_of(c), c.offset, mut=mut)
    u = tc.tol_units((bad.ess, bad.log_z), (good.ess, good.log_z))
    print(mut, name, u)
    assert max(u) >= 100.0, (mut, name, u)


# ---- the compaction -----------------------------------------------------------------------------------------------------------
SHAPES = tc.shapes()


def test_the_shape_list_is_the_stated_one():
    assert {s.B for s in SHAPES} == set(tc.B_LIST) and {s.D for s in SHAPES} == set(tc.D_LIST)
    assert any(s.D % 2 for s in SHAPES)
    for B in tc.B_ALL_PATTERNS:
        for n_in in (B, B - tc.BAIT_ROWS):
            assert {s.pattern for s in SHAPES if (s.B, s.D, s.n_in) == (B, 6, n_in)} == set(tc.PATTERNS)
    for B in tc.B_LIST:
        for D in tc.D_LIST:
            assert set(tc.THREE_PATTERNS) <= {s.pattern for s in SHAPES if (s.B, s.D) == (B, D)}
            if B > tc.BAIT_ROWS:
                assert {s.n_in for s in SHAPES if (s.B, s.D) == (B, D)} == {B, B - tc.BAIT_ROWS}
    assert {s.B for s in SHAPES if s.B > tc.TAIL_MAX_ROWS} == {2049, 4097}           # the separate kernels' first sizes
    # the one-launch form's LDS limit lies beyond every dimension a flow can have
    assert (3 * 64 + 4) * tc.TAIL_CHUNK * 4 <= tc.TAIL_LDS_BYTES < (3 * 127 + 4) * tc.TAIL_CHUNK * 4


def test_every_pattern_has_its_stated_survivors_and_every_kind_of_death_occurs():
    seen = set()
    for s in SHAPES:
        f = tc.point_fields(s)
        dead = tc.dead_mask(s)
        valid = np.isfinite(f["lq"]) & np.isfinite(f["lp"])
        assert np.array_equal(valid, ~dead), s                                   # the bait rows look alive
        assert int(valid[:s.n_in].sum()) == tc.survivors_stated(s), s
        seen |= set(f["kinds"][dead].tolist())
        for name in ("x", "lq"):                                          # distinct rows: a misplaced row shows
            a = f[name][valid].reshape(int(valid.sum()), 1 if f[name].ndim == 1 else s.D)
            assert np.unique(a, axis=0).shape[0] == a.shape[0], (s, name)
    assert seen == set(range(len(tc.KINDS)))
    q = {k[0]: (k[1], k[2]) for k in tc.KINDS}
    assert any(a is None and b is not None for a, b in q.values()) and any(a is not None and b is None for a, b in q.values())
    # the patterns that are there for one branch of the kernels
    s = tc.Shape(2049, 6, 2049, "first_1024")
    assert tc.dead_mask(s)[:1024].all() and not tc.dead_mask(s)[1024:].any()     # the first scan trip has no survivor
    assert tc.dead_mask(tc.Shape(2049, 6, 2049, "run_32_on_a_chunk"))[32:64].all()
    m = tc.dead_mask(tc.Shape(2049, 6, 2049, "run_33_across_chunks"))
    assert m.sum() == 33 and m[63] and m[64] and m[48] and m[80]
    assert tc.dead_mask(tc.Shape(2049, 6, 2049, "random_50pc")).sum() == 1024
    assert tc.dead_mask(tc.Shape(2049, 6, 2049, "all_but_last")).sum() == 2048    # a dead majority


@pytest.mark.parametrize("with_grad,extra", [(True, False), (False, False), (True, True), (False, True)])
def test_the_restated_compaction_is_field_of_mask_and_leaves_the_rest_alone(with_grad, extra):
    for s in SHAPES:
        if s.D not in (6, 7) and s.pattern != "alternating":
            continue
        f = tc.point_fields(s, with_grad, extra)
        valid = np.zeros(s.B, bool)
        valid[:s.n_in] = ~tc.dead_mask(s)[:s.n_in]
        outs = {form: tc.compact_restated(f, s.n_in, form) for form in ("in_place", "staged")}
        for form, (out, n_out, dest) in outs.items():
            assert n_out == int(valid.sum()) == tc.survivors_stated(s)
            assert np.array_equal(dest[dest >= 0], np.arange(n_out)) and np.array_equal(dest >= 0, valid[:s.n_in])
            for k in tc.FIELDS:
                if f[k] is None:
                    assert out[k] is None
                    continue
                assert np.array_equal(out[k][:n_out], f[k][valid], equal_nan=True), (s, form, k)
                assert np.array_equal(out[k][n_out:].view(np.int32), f[k][n_out:].view(np.int32)), (s, form, k)   # [n_out, B) untouched
        for k in tc.FIELDS:                                                        # the two forms: the same bits everywhere
            if f[k] is not None:
                assert np.array_equal(outs["in_place"][0][k].view(np.int32), outs["staged"][0][k].view(np.int32))
        if s.pattern == "all":
            assert outs["in_place"][1] == 0
            for k in tc.FIELDS:
                if f[k] is not None:
                    assert np.array_equal(outs["in_place"][0][k].view(np.int32), f[k].view(np.int32))    # nothing moves


# (mutant, shape that sees it, what differs: "dest" - an integer - or a field)
COMPACTION_MUTANTS = (("no_carry", tc.Shape(2049, 6, 2049, "alternating"), "dest"),
                      ("woff_le", tc.Shape(33, 6, 33, "row_0"), "dest"),
                      ("valid_lq_only", tc.Shape(33, 6, 33, "random_50pc"), "dest"),
                      ("valid_not_nan", tc.Shape(33, 6, 33, "random_50pc"), "dest"),
                      ("no_extra", tc.Shape(33, 6, 28, "alternating"), "extra"),
                      ("no_grad", tc.Shape(33, 6, 28, "alternating"), "gq"))


@pytest.mark.parametrize("mut,shape,what", COMPACTION_MUTANTS)
def test_one_line_mutants_of_the_restated_compaction_change_an_integer_or_a_field(mut, shape, what):
    assert shape in SHAPES
    f = tc.point_fields(shape, True, True)
    if what == "dest":
        good, bad = tc.ranks_restated(f["lq"], f["lp"], shape.n_in), tc.ranks_restated(f["lq"], f["lp"], shape.n_in, mut)
        assert not np.array_equal(good[0], bad[0])
    else:
        good, bad = tc.compact_restated(f, shape.n_in)[0], tc.compact_restated(f, shape.n_in, mut=mut)[0]
        assert not np.array_equal(good[what], bad[what])
        scale = np.abs(good[what]).max()
        assert np.abs(good[what] - bad[what]).max() >= 100 * 1e-5 * scale


# ---- the "chain init" tail's dead rows come from the base noise ------------------------------------------------------------------
@pytest.mark.parametrize("D", [6, 32])
def test_a_finite_base_noise_entry_kills_a_row_through_log_p_alone(D):
    nf = tc.init_flow(D)
    target = otgt.ManyWell(D)
    torch.manual_seed(1)
    eps0 = torch.randn(8, D)
    for r, v in enumerate(tc.INIT_POISONS):
        eps0[r, 0] = v
    with torch.no_grad():
        x, lq0 = nf.sample_eps(eps0)
        lq, lp = nf.log_prob(x), target.log_prob(x)
    assert not torch.isfinite(lq[:3]).any() or not torch.isfinite(lp[:3]).any()
    assert all(not (math.isfinite(lq[r]) and math.isfinite(lp[r])) for r in range(3))     # NaN, +inf, -inf: dead
    assert math.isfinite(lq[3]) and math.isfinite(lq0[3]) and not math.isfinite(lp[3])     # 3e10: dead through log_p alone
    assert torch.isfinite(lq[4:]).all() and torch.isfinite(lp[4:]).all()
    # the same with the finite poison in every coordinate (init_noise walks through them), one row each
    eps0 = torch.randn(D, D)
    eps0[torch.arange(D), torch.arange(D)] = tc.INIT_POISONS[3]
    with torch.no_grad():
        x, lq0 = nf.sample_eps(eps0)
        lq, lp = nf.log_prob(x), target.log_prob(x)
    assert torch.isfinite(lq).all() and torch.isfinite(lq0).all() and not torch.isfinite(lp).any()


@pytest.mark.parametrize("D", [6, 32])
def test_the_poisoned_base_noise_of_the_gpu_file_kills_exactly_its_rows(D):
    """init_noise as test_gpu_tail.py calls it (every B and pattern of (c)): through the oracle the dead rows are the pattern's, the
    clean noise kills none, and rows dead through log_p alone occur"""
    nf, target = tc.init_flow(D), otgt.ManyWell(D)
    for B in tc.INIT_B[:2] if D == 32 else tc.INIT_B:
        for pattern in tc.INIT_PATTERNS:
            clean, bad, dead = tc.init_noise(B, D, pattern)
            with torch.no_grad():
                res = []
                for eps in (clean, bad):
                    x, _ = nf.sample_eps(eps)
                    res.append((nf.log_prob(x), target.log_prob(x)))
            assert bool((torch.isfinite(res[0][0]) & torch.isfinite(res[0][1])).all())
            valid = torch.isfinite(res[1][0]) & torch.isfinite(res[1][1])
            assert np.array_equal(valid.numpy(), ~dead), (B, D, pattern)
            if dead.sum() >= len(tc.INIT_POISONS):
                assert bool((torch.isfinite(res[1][0]) & ~torch.isfinite(res[1][1])).any()), (B, D, pattern)
