"""CPU tests of the streaming multinomial resampler's specification (tests/resample_stream_spec.py) and of the host-side
refusals of its C ABI.  No GPU."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

import resample_stream_spec as spec
from oracle.numerical import fixed_point_weights, systematic_fixed


def _weights(n, seed=0, scale=2.0):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


# ---- properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ns", [(1, 1), (1, 7), (64, 64), (64, 5), (64, 1000), (1000, 333), (4097, 4097)])
def test_sorted_indices_are_monotone_and_in_range(n, ns):
    idx = spec.multinomial_stream(_weights(n, n), ns, seed=11)
    assert idx.shape == (ns,) and idx.dtype == np.int64
    assert idx.min() >= 0 and idx.max() < n
    assert np.all(np.diff(idx) >= 0)


def test_definition_by_128_bit_products():
    """point 3 as stated: first j with C_j * G_ns > G_k * total, in Python integers."""
    lw = _weights(300, 3)
    ns, seed = 500, 12345
    C = [int(c) for c in np.cumsum(fixed_point_weights(lw), dtype=np.uint64)]
    e = [int(v) for v in spec.spacings(seed, ns)]
    assert len(e) == ns + 1 and min(e) >= 1
    G = np.cumsum(np.array(e, dtype=object))
    want = [next(j for j, c in enumerate(C) if c * int(G[ns]) > int(G[k]) * C[-1]) for k in range(ns)]
    assert spec.multinomial_stream(lw, ns, seed).tolist() == want


def test_floor_muldiv_fast_path_is_exact():
    rng = np.random.default_rng(5)
    for total_bits in (1, 20, 42, 49):
        Gn = int(rng.integers(1 << 40, 1 << 61))
        G = rng.integers(1, Gn, size=2000).astype(np.uint64)
        total = int(rng.integers(1 << (total_bits - 1), 1 << total_bits))
        want = [(int(g) * total) // Gn for g in G]
        assert spec.floor_muldiv(G, total, Gn).tolist() == want
    # exact multiples (remainder 0) and the slow path
    assert spec.floor_muldiv(np.array([10, 20, 30], np.uint64), 7, 10).tolist() == [7, 14, 21]
    assert spec.floor_muldiv(np.array([3], np.uint64), (1 << 61) + 1, 7).tolist() == [(3 * ((1 << 61) + 1)) // 7]


def test_dead_rows_are_never_selected():
    lw = _weights(200, 1)
    dead = [0, 1, 2, 50, 51, 120, 198, 199]
    lw[dead[:3]] = -np.inf
    lw[dead[3:5]] = np.nan
    lw[dead[5]] = np.inf
    lw[dead[6:]] = -np.inf
    for order in ("sorted", "shuffled"):
        idx = spec.multinomial_stream(lw, 5000, seed=4, order=order)
        assert not np.isin(idx, dead).any()
        assert len(np.unique(idx)) > 100


def test_total_zero_convention():
    lw = np.full(17, -np.inf, dtype=np.float32)
    for order in ("sorted", "shuffled"):
        assert spec.multinomial_stream(lw, 9, seed=1, order=order).tolist() == [16] * 9


def test_seed_decides():
    lw = _weights(500, 2)
    a = spec.multinomial_stream(lw, 2000, seed=7)
    assert np.array_equal(a, spec.multinomial_stream(lw, 2000, seed=7))
    assert not np.array_equal(a, spec.multinomial_stream(lw, 2000, seed=8))
    assert np.array_equal(spec.multinomial_stream(lw, 2000, seed=-1), spec.multinomial_stream(lw, 2000, seed=(1 << 64) - 1))


@pytest.mark.parametrize("ns", [1, 2, 3, 5, 64, 1000, 4097])
def test_shuffled_is_a_permutation_of_sorted(ns):
    pi = spec.permutation(ns, seed=ns + 3)
    assert sorted(pi.tolist()) == list(range(ns))
    lw = _weights(333, ns)
    s = spec.multinomial_stream(lw, ns, seed=ns + 3, order="sorted")
    h = spec.multinomial_stream(lw, ns, seed=ns + 3, order="shuffled")
    assert np.array_equal(np.sort(h), s)
    assert np.array_equal(h, s[pi])
    if ns >= 64:
        assert not np.array_equal(pi, np.arange(ns))
        assert not np.array_equal(pi, spec.permutation(ns, seed=ns + 4))


def test_sample_bound():
    lw = _weights(8)
    with pytest.raises(AssertionError):
        spec.thresholds(lw, 0, 0)
    with pytest.raises(AssertionError):
        spec.thresholds(lw, spec.MAX_SAMPLES + 1, 0)
    # the largest spacing: y = 1 -> 32 ln 2
    assert int(spec.neg_log_fixed(np.array([0], np.uint64))[0]) == 32 * spec.LN2_FIX
    assert (spec.MAX_SAMPLES + 1) * 32 * spec.LN2_FIX < (1 << 62)
    assert (1 << 26) <= spec.MAX_SAMPLES


# ---- the fixed-point -ln -------------------------------------------------------------------------------------------
def test_log_polynomial_over_every_mantissa():
    """The measured part of the stated bound: |p(g - 1) - ln g| <= 5.2e-8 for every float32 g the reduction can produce."""
    f = (np.arange(1 << 23, 1 << 24, dtype=np.uint32).astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    g = np.where(f >= spec.SQRT2_F, f * np.float32(0.5), f).astype(np.float32)
    err = np.abs(spec.log_poly(g).astype(np.float64) - np.log(g.astype(np.float64)))
    assert err.max() <= 5.2e-8, err.max()


def test_fixed_point_neg_log_against_numpy():
    hi = np.array([0, 1, 2, 3, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xB504F333, 0xB504F334, 0xB5050000, 0xFFFFFFFE, 0xFFFFFFFF,
                   0x00000100, 0x000001FF, 0x00FFFFFF, 0x01000000], dtype=np.uint64)
    r = np.concatenate([hi << np.uint64(32), (hi << np.uint64(32)) | np.uint64(0xFFFFFFFF),
                        spec.stream_hash(99, np.arange(10 ** 6, dtype=np.uint64))])
    e = spec.neg_log_fixed(r)
    u = spec.uniform_of(r)
    assert e.min() >= 1 and int(e.max()) <= 32 * spec.LN2_FIX
    assert u.min() > 0.0 and u.max() < 1.0
    err = np.abs(e.astype(np.float64) * 2.0 ** -spec.FRAC_BITS + np.log(u))
    assert err.max() <= spec.LOG_BOUND, err.max()
    # the hashed uniforms look uniform, the spacings exponential (mean 1, variance 1) at the 1e-6 level of 10^6 draws
    uu, ee = u[-10 ** 6:], e[-10 ** 6:].astype(np.float64) * 2.0 ** -spec.FRAC_BITS
    assert abs(uu.mean() - 0.5) < 5 * np.sqrt(1 / 12e6)
    assert abs(ee.mean() - 1.0) < 5e-3 and abs(ee.var() - 1.0) < 2e-2
    assert stats.kstest(uu, "uniform").pvalue > 1e-6


# ---- distribution --------------------------------------------------------------------------------------------------
def test_counts_are_multinomial_not_stratified():
    n, ns, n_seeds = 64, 50_000, 300
    lw = _weights(n, 0, 2.0)
    W = fixed_point_weights(lw).astype(np.float64)
    p = W / W.sum()
    counts = np.stack([np.bincount(spec.multinomial_stream(lw, ns, seed=1000 + s), minlength=n) for s in range(n_seeds)])
    assert np.all(counts.sum(axis=1) == ns)
    # (a) pooled chi-square of the counts
    chi2 = (((counts - ns * p) ** 2) / (ns * p)).sum()
    limit = stats.chi2.ppf(1 - 1e-6, (n - 1) * n_seeds)
    print(f"pooled chi2 {chi2:.1f}  dof {(n - 1) * n_seeds}  limit {limit:.1f}")
    assert chi2 < limit
    # (b) variance of the heaviest particle's count over the seeds: multinomial ns p (1 - p), not a stratified sampler's < 1
    j = int(np.argmax(p))
    var0 = ns * p[j] * (1 - p[j])
    dof = n_seeds - 1
    lo, hi = stats.chi2.ppf(0.5e-6, dof) * var0 / dof, stats.chi2.ppf(1 - 0.5e-6, dof) * var0 / dof
    var = counts[:, j].var(ddof=1)
    u0 = np.random.default_rng(1).random(n_seeds)
    var_sys = np.array([np.bincount(systematic_fixed(lw, float(u), ns), minlength=n)[j] for u in u0]).var(ddof=1)
    print(f"heaviest p {p[j]:.4f}: var {var:.1f} in [{lo:.1f}, {hi:.1f}] (multinomial {var0:.1f}); systematic {var_sys:.3f}")
    assert lo < var < hi
    assert not (lo < var_sys < hi)


# ---- binding without a GPU -----------------------------------------------------------------------------------------
def test_cabi_symbols_and_refusals():
    from fab_torch_amd import _lib
    assert "fabhip_resample_stream_workspace_bytes" in _lib.SYMBOLS
    assert "fabhip_resample_multinomial_stream" in _lib.SYMBOLS
    lib = _lib.load()
    wsb = lib.fabhip_resample_stream_workspace_bytes
    assert wsb(1 << 20, 1 << 10) > wsb(1 << 10, 1 << 10)
    assert wsb(1 << 10, 1 << 20) > wsb(1 << 10, 1 << 10)
    assert wsb(0, 5) == 0 and wsb(5, 0) == 0
    f = lib.fabhip_resample_multinomial_stream
    EINVAL, ENOSPC = -1, -4
    assert lib.fabhip_strerror(EINVAL).startswith(b"invalid") and lib.fabhip_strerror(ENOSPC).startswith(b"workspace")
    fake = C.c_void_p(1 << 20)                    # never dereferenced: every call below is refused before any launch
    n, ns = 1000, 500
    nb = wsb(n, ns)

    def call(log_w=fake, n=n, seed=1, ns=ns, order=0, idx=fake, ws=fake, nb=nb):
        return f(log_w, n, seed, ns, order, idx, ws, nb, None)

    assert call(log_w=None) == EINVAL
    assert call(idx=None) == EINVAL
    assert call(ws=None) == EINVAL
    assert call(n=0) == EINVAL
    assert call(ns=0) == EINVAL
    assert call(order=2) == EINVAL and call(order=-1) == EINVAL
    assert call(ns=spec.MAX_SAMPLES + 1, nb=1 << 40) == EINVAL
    assert call(ws=C.c_void_p((1 << 20) + 8)) == EINVAL          # workspace must be 256-byte aligned
    assert call(nb=nb - 1) == ENOSPC
