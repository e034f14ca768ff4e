"""CPU tests of the specification of the seeded stratified resampler (tests/resample_stratified_spec.py): they pin the spec
before tests/test_gpu_resample_stratified.py and tests/test_gpu_smc_stratified.py pin the device to it.  Inputs: the cases of
tests/resample_fixed_cases.py with every n_samples they list."""
import functools

import numpy as np
import pytest

import resample_fixed_cases as rc
import resample_stratified_spec as spec
import resample_stream_spec as stream
import smc_spec
from oracle import numerical as onum

SEEDS = (0, 1, 0xDEADBEEFCAFEF00D, (1 << 64) - 1)
SPECIAL_NAMES = ("unaligned", "one_survivor", "heavy_tail", "mixed", "hot_wave", "few_weights_many_draws", "list_full", "no_list",
                 "dead_middle", "all_equal", "all_dead", "nan_inf")


def _weights(case):
    C = rc.expected_cdf(case)
    return C, np.diff(np.concatenate([[0], C.astype(np.int64)]))


def _count_bound_ok(counts, W, total, ns):
    """floor(ns W_j / total) - 1 <= count_j <= ceil(ns W_j / total) + 1 in integers (Python ints: ns W_j reaches 2^83)."""
    prod = W.astype(object) * int(ns)
    lo = np.array([p // total - 1 for p in prod], dtype=np.int64)
    hi = np.array([-((-p) // total) + 1 for p in prod], dtype=np.int64)
    return bool(np.all(counts >= lo) and np.all(counts <= hi))


@pytest.mark.parametrize("name", rc.EDGE_NAMES)
def test_indices_counts_and_closed_form_inverse(name):
    """Non-decreasing indices below n, dead rows never drawn, the count bound, and K(C_j) of the closed form = the number of
    thresholds below C_j (the arithmetic the kernel evaluates instead of a search)."""
    case = rc.get_case(name)
    n = len(case.log_w)
    C, W = _weights(case)
    total = int(C[-1])
    for ns in case.ns:
        for seed in SEEDS:
            idx = spec.stratified(case.log_w, ns, seed)
            assert idx.shape == (ns,) and idx.dtype == np.int64
            assert idx.min() >= 0 and idx.max() < n and np.all(np.diff(idx) >= 0)
            assert np.all(W[idx] > 0)
            counts = np.bincount(idx, minlength=n)
            assert _count_bound_ok(counts, W, total, ns), (name, ns, seed)
            assert np.abs(counts - ns * W.astype(np.float64) / total).max() < 2.0
            K = spec.closed_form_K(C, ns, seed)
            np.testing.assert_array_equal(np.diff(np.concatenate([[0], K])), counts, err_msg=f"{name} ns={ns} seed={seed}")
            assert K[-1] == ns
            t = spec.thresholds(total, ns, seed)
            np.testing.assert_array_equal(K, np.searchsorted(t, C, side="left"))


def test_all_dead_gives_the_last_index():
    case = rc.get_case("all_dead")
    for ns in case.ns:
        assert (spec.stratified(case.log_w, ns, 5) == len(case.log_w) - 1).all()
        assert (spec.stratified(case.log_w, ns, 5, "shuffled") == len(case.log_w) - 1).all()


@pytest.mark.parametrize("n", [1, 17, 257, 1025, 4097])
def test_equal_weights_and_ns_equal_n_is_the_identity(n):
    for seed in SEEDS:
        np.testing.assert_array_equal(spec.stratified(np.zeros(n, np.float32), n, seed), np.arange(n))


def test_unbiased_on_edge_257():
    """2000 seeds: every mean count within 5 standard errors of ns w_j.  An item covers at most two strata partly, each a
    Bernoulli of variance <= 1/4, so the variance of a count is <= 1/2.  (Measured: the largest deviation is 1.70 standard
    errors.)"""
    case = rc.get_case("edge_257")
    C, W = _weights(case)
    ns, reps = 257, 2000
    acc = np.zeros(len(W), np.float64)
    for s in range(reps):
        acc += np.bincount(spec.indices_from_cdf(C, ns, s * 0x1234567 + 99), minlength=len(W))
    dev = np.abs(acc / reps - ns * W.astype(np.float64) / float(C[-1])) / np.sqrt(0.5 / reps)
    print(f"largest deviation: {dev.max():.2f} standard errors")
    assert dev.max() <= 5.0


def test_offsets_are_not_systematic():
    ns = 4096
    C = onum.fixed_point_cdf(np.zeros(ns, np.float32))
    F, S = spec.strata(int(C[-1]), ns)
    for seed in SEEDS:
        U = spec.offsets(seed, np.arange(ns, dtype=np.uint64), S)
        assert int(U.max()) < S
        frac = U.astype(np.float64) / float(S)
        assert len(np.unique(U)) > ns // 2 and 0.45 <= frac.mean() <= 0.55
    # mulhi64 against Python integers
    h = stream.stream_hash(7, np.arange(64, dtype=np.uint64))
    for b in (S, 1, (1 << 64) - 1, 0x123456789ABCDEF):
        np.testing.assert_array_equal(spec.mulhi64(h, b), np.array([(int(x) * b) >> 64 for x in h], dtype=np.uint64))


@pytest.mark.parametrize("name", ["edge_17", "edge_1025", "edge_4097"])
def test_shuffled_is_the_keyed_permutation_of_sorted(name):
    case = rc.get_case(name)
    for ns in case.ns:
        a = spec.stratified(case.log_w, ns, 42, "sorted")
        b = spec.stratified(case.log_w, ns, 42, "shuffled")
        np.testing.assert_array_equal(np.sort(b), a)
        np.testing.assert_array_equal(b, a[stream.permutation(ns, 42)])


def test_limits_are_stated():
    assert spec.MAX_SAMPLES == (1 << 31) - 3
    with pytest.raises(AssertionError):
        spec.strata(1 << 40, 0)
    with pytest.raises(AssertionError):
        spec.strata(1 << 40, spec.MAX_SAMPLES + 1)
    # k S + U_k stays below 2^62 at the largest n_samples and the largest total
    for total in ((1 << 62) - 1, 1, (1 << 36) * 70_001):
        F, S = spec.strata(total, spec.MAX_SAMPLES)
        assert spec.MAX_SAMPLES * S <= total << F < 1 << 62 and S >= 1 << 30


# ---- the estimates of the kernel (csrc/resample_emit.hip: stratified_rel / stratified_rel_small) --------------------------
def _wave_estimates(C, ns):
    """Per wave tile: (T bound, |estimate - exact| of the fp32 quotient relative to the wave's stratum q0, the same for the
    float64 quotient) - the exact step that follows corrects a miss of ONE stratum, not more."""
    total = int(C[-1])
    F, S = spec.strata(total, ns)
    invS_f, invS = np.float32(1) / np.float32(S), 1.0 / float(S)
    out = []
    for w0 in range(0, len(C), rc.EM_WAVE_ITEMS):
        c_start = int(C[w0 - 1]) if w0 else 0
        Cw = C[w0:w0 + rc.EM_WAVE_ITEMS]
        B0 = c_start << F
        q0 = B0 // S
        Bw = B0 - q0 * S
        d = Cw - np.uint64(c_start)
        X = np.uint64(Bw) + (d << np.uint64(F))
        exact_rel = (X // np.uint64(S)).astype(np.int64)
        xf = ((X >> np.uint64(32)).astype(np.float32) * np.float32(4294967296.0)).astype(np.float32)
        xf = (xf + (X & np.uint64(0xFFFFFFFF)).astype(np.float32)).astype(np.float32)
        k32 = (xf * invS_f).astype(np.float32).astype(np.int64)
        y = (d.astype(np.float64) * float(1 << F) + float(B0)) * invS
        k64 = y.astype(np.int64)
        exact_abs = ((Cw << np.uint64(F)) // np.uint64(S)).astype(np.int64)
        out.append((int(exact_rel[-1]), int(np.abs(k32 - exact_rel).max()), int(np.abs(k64 - exact_abs).max())))
    return out


@pytest.mark.parametrize("name", ["edge_1025", "edge_4097", "edge_65537", "heavy_tail", "mixed", "hot_wave", "all_equal",
                                  "few_weights_many_draws", "one_survivor"])
def test_quotient_estimates_miss_by_at_most_one_stratum(name):
    case = rc.get_case(name)
    C = rc.expected_cdf(case)
    for ns in case.ns:
        for span, e32, e64 in _wave_estimates(C, ns):
            assert e64 <= 1, (name, ns, e64)
            if span + 1 < rc.EM_F64_STRATA:              # the fp32 estimate is used while the wave owns fewer than 2^20 strata
                assert e32 <= 1, (name, ns, span, e32)


# ---- every special case still reaches the branch it is listed for, under stratified thresholds ----------------------------
def stratified_profile(log_w, ns, seed):
    """rc.branch_profile's per-wave quantities from the stratified spec's output.  `capacity`: the stratified entry point carves
    its run list for n_samples / EM_GIANT + 1 runs (more than can exist), so the list is never full and never absent."""
    n = len(log_w)
    C = onum.fixed_point_cdf(log_w)
    nw = (n + rc.EM_WAVE_ITEMS - 1) // rc.EM_WAVE_ITEMS
    prof = {"total": int(C[-1]), "capacity": ns // rc.EM_GIANT + 1}
    counts = np.zeros(nw * rc.EM_WAVE_ITEMS, np.int64)
    if prof["total"] > 0:
        counts[:n] = np.bincount(spec.indices_from_cdf(C, ns, seed), minlength=n)
    counts = counts.reshape(nw, rc.EM_WAVE_ITEMS)
    prof.update(strata=counts.sum(1), longest=counts.max(1), giants=(counts >= rc.EM_GIANT).sum(1), distinct=(counts > 0).sum(1))
    return prof


# the seeds tests/test_gpu_resample_stratified.py draws with: (special cases, edge sizes), first and second seed of each
GPU_SEEDS = ((0xC0FFEE, 0xDEADBEEFCAFEF00D), ((1 << 64) - 1, 0))


@functools.lru_cache(maxsize=None)
def _profiles(seed_special, seed_edge):
    return {(name, ns): stratified_profile(rc.get_case(name).log_w, ns, seed_edge if name.startswith("edge_") else seed_special)
            for name in SPECIAL_NAMES + rc.EDGE_NAMES for ns in rc.get_case(name).ns}


@pytest.mark.parametrize("seeds", GPU_SEEDS)
def test_special_cases_reach_their_branches_under_stratified_thresholds(seeds):
    """Judged from the spec's output for exactly the (case, n_samples, seed) runs of the GPU file."""
    P = _profiles(*seeds)
    n = rc.SPECIAL_N
    # one run holds every stratum: published, every window skipped; the float64 estimate at the larger n_samples
    p = P[("one_survivor", n)]
    assert p["giants"].sum() == 1 and p["distinct"].sum() == 1
    assert P[("one_survivor", (1 << 20) + 4097)]["strata"].max() >= rc.EM_F64_STRATA
    # giant runs beside other runs of the same wave (they start / end inside a window)
    assert P[("heavy_tail", n)]["giants"].sum() == 1 and P[("heavy_tail", 3 * n + 5)]["giants"].sum() == 2
    assert P[("heavy_tail", (1 << 21) + 3)]["strata"].max() >= rc.EM_F64_STRATA
    p = P[("mixed", 3 * n + 5)]
    assert bool(((p["giants"] >= 1) & (p["distinct"] >= p["giants"] + 100)).any())
    # a wave that enters the giant branch and finds no giant run; at 16 n + 3 the float64 estimate on ~1000 distinct runs
    p = P[("hot_wave", n)]
    assert bool(((p["strata"] >= rc.EM_GIANT) & (p["giants"] == 0)).any())
    p = P[("hot_wave", 16 * n + 3)]
    assert bool(((p["strata"] >= rc.EM_F64_STRATA) & (p["distinct"] >= 100)).any())
    # a ragged last wave that owns every stratum, float64 estimate
    p = P[("few_weights_many_draws", (1 << 20) + 5)]
    assert len(p["strata"]) == 1 and p["strata"][0] == (1 << 20) + 5
    # several published runs in one wave (the systematic entry point's list is full / absent here; this one's holds them all)
    for key in (("list_full", 480_000), ("no_list", 200_000)):
        assert 1 < P[key]["giants"].sum() <= P[key]["capacity"]
    # waves without a stratum
    p = P[("dead_middle", n)]
    assert (p["strata"] == 0).sum() >= 40
    assert P[("all_dead", n)]["total"] == 0 and all(P[(k, n)]["total"] > 0 for k in ("nan_inf", "all_equal", "unaligned"))
    # several marker windows below the giant threshold
    assert any(bool(((p["strata"] > rc.EM_WIN) & (p["strata"] < rc.EM_GIANT) & (p["giants"] == 0)).any())
               for (name, _), p in P.items() if name.startswith("edge_"))


@pytest.mark.parametrize("name", SPECIAL_NAMES)
def test_special_cases_obey_the_count_bound(name):
    case = rc.get_case(name)
    C, W = _weights(case)
    total = int(C[-1])
    if total == 0:
        return
    for ns in case.ns:
        idx = spec.indices_from_cdf(C, ns, 0xC0FFEE)
        counts = np.bincount(idx, minlength=len(W))
        assert np.all(np.diff(idx) >= 0) and _count_bound_ok(counts, W, total, ns)
        np.testing.assert_array_equal(np.diff(np.concatenate([[0], spec.closed_form_K(C, ns, 0xC0FFEE)])), counts)


# ---- inside the SMC mode ---------------------------------------------------------------------------------------------------
def test_smc_decision_is_unchanged_and_the_ancestors_are_stratified():
    rng = np.random.default_rng(3)
    lw = (rng.standard_normal(101) * 2).astype(np.float32)
    lw[7] = -np.inf
    lw[50] = np.nan
    for tau, u in ((1.5, 0.37), (0.5, 0.0), (1.5, float(np.nextafter(1.0, 0.0))), (0.01, 0.6)):
        a, b = smc_spec.decide(lw, tau, u), spec.decide(lw, tau, u)
        assert a.resampled == b.resampled and a.ess == b.ess
        assert (a.log_w_common == b.log_w_common) or (np.isnan(a.log_w_common) and np.isnan(b.log_w_common))
        if not a.resampled:
            np.testing.assert_array_equal(a.ancestors, b.ancestors)
            continue
        assert not np.array_equal(a.ancestors, b.ancestors)
        np.testing.assert_array_equal(b.ancestors, spec.stratified(lw, len(lw), spec.seed_of_uniform(u)))
        C = onum.fixed_point_cdf(lw)
        W = np.diff(np.concatenate([[0], C.astype(np.int64)]))
        assert _count_bound_ok(np.bincount(b.ancestors, minlength=len(lw)), W, int(C[-1]), len(lw))
    assert spec.seed_of_uniform(0.0) == 0 and spec.seed_of_uniform(1.0) == 0 and spec.seed_of_uniform(-0.5) == 0
    assert spec.seed_of_uniform(float("nan")) == 0 and spec.seed_of_uniform(0.5) == 0x3FE0000000000000


# ---- sharded chains: the resampling step over ranks is systematic ---------------------------------------------------------
def test_sharded_sampler_refuses_a_stratified_sampler():
    """No GPU, no process group: the refusal comes before anything is enqueued."""
    from fab_torch_amd import _ops, parallel

    class _Ais:
        resample_threshold, resample_method = 0.5, "stratified"

    class _Backend:
        hmc, tuning, ais = True, False, _Ais()

        def run_fused(self, *a, **k):
            raise AssertionError("not reached: the sampler is refused first")

    sh = parallel.ShardedAnnealedImportanceSampler(backend=_Backend(), resample_across_ranks=True)
    with pytest.raises(_ops.FabhipError, match="resample_method"):
        sh.sample_and_log_weights(64)
    # without resampling over ranks the existing refusal of the threshold comes first, as before
    sh = parallel.ShardedAnnealedImportanceSampler(backend=_Backend(), resample_across_ranks=False)
    with pytest.raises(_ops.FabhipError, match="resample_threshold"):
        sh.sample_and_log_weights(64)
