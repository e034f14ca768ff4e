"""GPU tests of the seeded streaming multinomial resampler (fabhip_resample_multinomial_stream) against its specification
(tests/resample_stream_spec.py): the device follows the spec bit for bit."""
import numpy as np
import pytest
import torch

import resample_stream_spec as spec

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from oracle.numerical import fixed_point_weights     # noqa: E402

DEV = "cuda"
EDGE_N = [1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537, 300_001]


def _check(lw, lw_d, ns, seed, orders=("sorted", "shuffled")):
    want = spec.multinomial_stream(lw, ns, seed, "sorted")
    pi = spec.permutation(ns, seed) if "shuffled" in orders else None
    for order in orders:
        got = fa.multinomial_stream_indices(lw_d, n_samples=ns, seed=seed, order=order).cpu().numpy()
        np.testing.assert_array_equal(got, want if order == "sorted" else want[pi], err_msg=f"n={len(lw)} ns={ns} {order}")


@pytest.mark.parametrize("N", EDGE_N)
def test_edge_sizes_bit_exact_vs_spec(N):
    """Sizes around every lane-row / wave-tile / block boundary, more and fewer draws than weights, zero-weight runs at both
    ends, both orders."""
    rng = np.random.default_rng(2000 + N)
    lw = (rng.standard_normal(N) * 2.5).astype(np.float32)
    if N > 40:
        lw[: N // 9] = -np.inf
        lw[-(N // 11):] = -np.inf
    lw_d = torch.tensor(lw).to(DEV)
    for i, ns in enumerate((N, 3 * N + 5, max(1, N // 3), 1, 63, 64, 65)):
        _check(lw, lw_d, ns, seed=77 * N + i)


@pytest.mark.parametrize("case", ["unaligned", "one_survivor", "heavy_tail", "mixed", "all_equal", "all_dead", "nan_inf"])
def test_special_weights_bit_exact_vs_spec(case):
    """A log_w pointer that is not 16-byte aligned; one weight holding all the mass and two weights holding most of it (runs
    long enough for the grid-wide fill); all weights equal; all weights dead (every index n - 1); NaN / +inf rows weigh 0."""
    rng = np.random.default_rng(sum(map(ord, case)))
    N = 300_001
    lw = (rng.standard_normal(N) * 2).astype(np.float32)
    if case == "one_survivor":
        lw[:] = -np.inf; lw[43210] = 0.5
    elif case == "heavy_tail":
        lw[12345] = 40.0; lw[266000] = 38.5
    elif case == "mixed":
        lw[12345] = 12.0; lw[200000] = 11.5
    elif case == "all_equal":
        lw[:] = 1.25
    elif case == "all_dead":
        lw[:] = -np.inf
    elif case == "nan_inf":
        lw[20000:23000] = np.nan; lw[100:200] = np.inf; lw[-5000:] = -np.inf
    lw_d = torch.tensor(lw).to(DEV)
    if case == "unaligned":
        buf = torch.empty(N + 1, device=DEV); buf[1:] = lw_d; lw_d = buf[1:]
        assert lw_d.data_ptr() % 16 != 0
    for ns in (N, 3 * N + 5, 70_000):
        _check(lw, lw_d, ns, seed=0xC0FFEE + ns)
    if case == "all_dead":
        assert (fa.multinomial_stream_indices(lw_d, n_samples=77, seed=1).cpu().numpy() == N - 1).all()


def test_2_pow_20_bit_exact_vs_spec():
    N = 1 << 20
    lw = (np.random.default_rng(5).standard_normal(N) * 3).astype(np.float32)
    _check(lw, torch.tensor(lw).to(DEV), N, seed=-123456789)


def test_2_pow_26_against_the_spec_at_chosen_positions():
    """N = ns = 2^26, heavy-tailed and flat weights: non-decreasing, counts sum to ns, 2^16 draw positions agree exactly with the
    spec evaluated for those positions only; the sorted copy of the shuffled output is the sorted output."""
    N = 1 << 26
    seed = 20260101
    G = np.cumsum(spec.spacings(seed, N), dtype=np.uint64)
    Gn = int(G[-1])
    pos = np.unique(np.concatenate([np.random.default_rng(9).integers(0, N, size=(1 << 16) - 4), [0, 1, N - 2, N - 1]]))
    Gk = G[pos]
    del G
    g = torch.Generator(device=DEV).manual_seed(0)
    for sigma in (3.0, 0.0):
        lw_d = torch.randn(N, device=DEV, generator=g) * sigma
        a = fa.multinomial_stream_indices(lw_d, seed=seed)
        assert a.shape == (N,) and bool((a[1:] >= a[:-1]).all()) and int(a.min()) >= 0 and int(a.max()) < N
        assert int(torch.bincount(a, minlength=N).sum()) == N
        C = np.cumsum(fixed_point_weights(lw_d.cpu().numpy()), dtype=np.uint64)
        t = spec.floor_muldiv(Gk, int(C[-1]), Gn)
        want = np.searchsorted(C, t, side="right").astype(np.int64)
        del C
        np.testing.assert_array_equal(a[torch.tensor(pos, device=DEV)].cpu().numpy(), want)
        if sigma == 3.0:
            b = fa.multinomial_stream_indices(lw_d, seed=seed, order="shuffled")
            assert not torch.equal(a, b)
            assert torch.equal(torch.sort(b).values, a)
            del b
        del a, lw_d


def test_determinism_streams_stale_workspace_and_graph():
    N = 200_000
    lw = torch.randn(N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) * 2.5
    for order in ("sorted", "shuffled"):
        a = fa.multinomial_stream_indices(lw, seed=42, order=order)
        assert torch.equal(a, fa.multinomial_stream_indices(lw, seed=42, order=order))
        assert not torch.equal(a, fa.multinomial_stream_indices(lw, seed=43, order=order))
        # a preceding call of another size leaves other bytes in the scratch
        fa.multinomial_stream_indices(torch.randn(3 * N + 11, device=DEV), n_samples=777, seed=1, order=order)
        fa.multinomial_stream_indices(lw[:1234], n_samples=5 * N, seed=2, order=order)
        assert torch.equal(a, fa.multinomial_stream_indices(lw, seed=42, order=order))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            b = fa.multinomial_stream_indices(lw, seed=42, order=order)
        torch.cuda.current_stream().wait_stream(s)
        assert torch.equal(a, b)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c = fa.multinomial_stream_indices(lw, seed=42, order=order)
        c.fill_(-1)
        g.replay(); torch.cuda.synchronize()
        assert torch.equal(a, c)
        c.fill_(-1)
        g.replay(); torch.cuda.synchronize()
        assert torch.equal(a, c)


def test_seed_none_draws_from_the_cpu_generator():
    lw = torch.randn(5000, device=DEV)
    torch.manual_seed(11)
    a = fa.multinomial_stream_indices(lw)
    b = fa.multinomial_stream_indices(lw)
    torch.manual_seed(11)
    assert torch.equal(a, fa.multinomial_stream_indices(lw)) and not torch.equal(a, b)
    with pytest.raises(Exception):
        fa.multinomial_stream_indices(lw, seed=1, order="random")
    with pytest.raises(Exception):
        fa.multinomial_stream_indices(lw.cpu(), seed=1)


def test_resample_with_the_new_method_and_unchanged_default():
    B, D = 3000, 6
    torch.manual_seed(0)
    x = torch.randn(B, D, device=DEV)
    lw = torch.randn(B, device=DEV) * 2
    p = fa.Point(x, torch.randn(B, device=DEV), torch.randn(B, device=DEV), torch.randn(B, D, device=DEV), torch.randn(B, D, device=DEV))
    idx = fa.multinomial_stream_indices(lw, seed=99)
    np.testing.assert_array_equal(idx.cpu().numpy(), spec.multinomial_stream(lw.cpu().numpy(), B, 99))
    r = fa.resample(p, lw, method="multinomial_stream", seed=99)
    for got, src in ((r.x, p.x), (r.log_q, p.log_q), (r.log_p, p.log_p), (r.grad_log_q, p.grad_log_q), (r.grad_log_p, p.grad_log_p)):
        assert torch.equal(got, src[idx])
    assert torch.equal(fa.resample(x, lw, method="multinomial_stream", seed=99), x[idx])
    # the default method is what it was: float64 uniforms from the device generator -> fabhip_resample_multinomial
    torch.manual_seed(5)
    got = fa.resample(x, lw)
    torch.manual_seed(5)
    u = torch.rand(B, dtype=torch.float64, device=DEV)
    assert torch.equal(got, x[fa.multinomial_indices(lw, u=u)])
    torch.manual_seed(5)
    assert torch.equal(got, fa.resample(x, lw, method="multinomial"))
