"""GPU tests of the seeded stratified resampler (fabhip_resample_stratified) against its specification
(tests/resample_stratified_spec.py): the device follows the spec bit for bit.  Inputs: the named cases of
tests/resample_fixed_cases.py (tests/test_resample_stratified_spec.py shows which branch of the emitter each one reaches)."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_fixed_cases as rc
import resample_stratified_spec as spec
import resample_stream_spec as stream

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _lib            # noqa: E402

DEV = "cuda"
SPECIAL_NAMES = ("unaligned", "one_survivor", "heavy_tail", "mixed", "hot_wave", "few_weights_many_draws", "list_full", "no_list",
                 "dead_middle", "all_equal", "all_dead", "nan_inf")


def _device_log_w(case):
    lw = torch.tensor(case.log_w).to(DEV)
    if case.unaligned:
        buf = torch.empty(len(case.log_w) + 1, device=DEV)
        buf[1:] = lw
        lw = buf[1:]
        assert lw.data_ptr() % 16 != 0
    return lw


def _check_case(name, seeds):
    case = rc.get_case(name)
    C_ = rc.expected_cdf(case)
    lw_d = _device_log_w(case)
    for ns in case.ns:
        for seed in seeds:
            want = spec.indices_from_cdf(C_, ns, seed)
            got = fa.stratified_indices(lw_d, n_samples=ns, seed=seed).cpu().numpy()
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, f"{name} ns={ns} seed={seed:#x}: {bad.size} indices differ, first at draw {bad[0]}: " \
                                  f"{got[bad[0]]} vs {want[bad[0]]}"


@pytest.mark.parametrize("name", rc.EDGE_NAMES)
def test_edge_sizes_bit_exact_vs_spec(name):
    """Sizes around every lane-row / wave-tile / block boundary, n_samples of 1, around 64, fewer and more than the weights,
    zero-weight runs at both ends."""
    _check_case(name, (0xDEADBEEFCAFEF00D, 0))


@pytest.mark.parametrize("name", SPECIAL_NAMES)
def test_special_weights_bit_exact_vs_spec(name):
    """Giant runs (published and filled grid-wide), a wave that owns >= 2^20 strata (float64 estimate), ragged last waves,
    zero-weight waves, an unaligned log_w pointer, all weights dead, non-finite rows."""
    _check_case(name, (0xC0FFEE, (1 << 64) - 1))


def test_2_pow_20_bit_exact_vs_spec():
    N = 1 << 20
    lw = (np.random.default_rng(5).standard_normal(N) * 3).astype(np.float32)
    got = fa.stratified_indices(torch.tensor(lw).to(DEV), seed=-123456789).cpu().numpy()
    np.testing.assert_array_equal(got, spec.stratified(lw, N, (-123456789) & ((1 << 64) - 1)))


@pytest.mark.parametrize("name", ["edge_17", "edge_1025", "edge_16385"])
def test_shuffled_order_bit_exact_vs_spec(name):
    case = rc.get_case(name)
    lw_d = torch.tensor(case.log_w).to(DEV)
    for ns in case.ns:
        want = spec.stratified(case.log_w, ns, 42, "sorted")[stream.permutation(ns, 42)]
        got = fa.stratified_indices(lw_d, n_samples=ns, seed=42, order="shuffled").cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"{name} ns={ns}")


def test_determinism_streams_stale_workspace_and_graph():
    N = 200_000
    lw = torch.randn(N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)) * 2.5
    for order in ("sorted", "shuffled"):
        a = fa.stratified_indices(lw, seed=42, order=order)
        assert torch.equal(a, fa.stratified_indices(lw, seed=42, order=order))
        assert not torch.equal(a, fa.stratified_indices(lw, seed=43, order=order))
        # a preceding call of another size leaves other bytes in the scratch
        fa.stratified_indices(torch.randn(3 * N + 11, device=DEV), n_samples=777, seed=1, order=order)
        fa.stratified_indices(lw[:1234], n_samples=5 * N, seed=2, order=order)
        assert torch.equal(a, fa.stratified_indices(lw, seed=42, order=order))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            b = fa.stratified_indices(lw, seed=42, order=order)
        torch.cuda.current_stream().wait_stream(s)
        assert torch.equal(a, b)
        g = torch.cuda.CUDAGraph()                      # (one stream: no parallel branches)
        with torch.cuda.graph(g):
            c = fa.stratified_indices(lw, seed=42, order=order)
        for _ in range(2):
            c.fill_(-1)
            g.replay(); torch.cuda.synchronize()
            assert torch.equal(a, c)


def test_seed_none_draws_from_the_cpu_generator_and_refusals():
    lw = torch.randn(5000, device=DEV)
    torch.manual_seed(11)
    a = fa.stratified_indices(lw)
    b = fa.stratified_indices(lw)
    torch.manual_seed(11)
    assert torch.equal(a, fa.stratified_indices(lw)) and not torch.equal(a, b)
    with pytest.raises(Exception):
        fa.stratified_indices(lw, seed=1, order="random")
    with pytest.raises(Exception):
        fa.stratified_indices(lw.cpu(), seed=1)
    with pytest.raises(Exception):
        fa.stratified_indices(lw, n_samples=0, seed=1)


def test_resample_with_the_new_method_and_unchanged_default():
    B, D = 3000, 6
    torch.manual_seed(0)
    x = torch.randn(B, D, device=DEV)
    lw = torch.randn(B, device=DEV) * 2
    p = fa.Point(x, torch.randn(B, device=DEV), torch.randn(B, device=DEV), torch.randn(B, D, device=DEV), torch.randn(B, D, device=DEV))
    want = torch.tensor(spec.stratified(lw.cpu().numpy(), B, 99), device=DEV)
    assert torch.equal(fa.stratified_indices(lw, seed=99), want)
    r = fa.resample(p, lw, method="stratified", seed=99)
    for got, src in ((r.x, p.x), (r.log_q, p.log_q), (r.log_p, p.log_p), (r.grad_log_q, p.grad_log_q), (r.grad_log_p, p.grad_log_p)):
        assert torch.equal(got, src[want])
    assert torch.equal(fa.resample(x, lw, method="stratified", seed=99), x[want])
    # the seed decides, not torch's generators (the systematic resampler would draw its u0 from the CPU generator)
    torch.manual_seed(1)
    assert torch.equal(fa.resample(x, lw, method="stratified", seed=99), x[want])
    # the default method is what it was: float64 uniforms from the device generator -> fabhip_resample_multinomial
    torch.manual_seed(5)
    got = fa.resample(x, lw)
    torch.manual_seed(5)
    u = torch.rand(B, dtype=torch.float64, device=DEV)
    assert torch.equal(got, x[fa.multinomial_indices(lw, u=u)])
    torch.manual_seed(5)
    u0 = float(torch.rand((), dtype=torch.float64))
    torch.manual_seed(5)
    assert torch.equal(fa.resample(x, lw, method="systematic"), x[fa.systematic_indices(lw, u0=u0)])


def test_c_abi_error_codes_and_workspace_size():
    lib = _lib.load()
    n, ns = 5000, 7000
    size = lib.fabhip_resample_stratified_workspace_bytes
    nb = size(n, ns)
    assert nb >= 8 * ns and nb % 256 == 0
    assert size(0, ns) == 0 and size(n, 0) == 0 and size(n, (1 << 31) - 2) == 0 and size(n, (1 << 31) - 3) > 8 * ((1 << 31) - 3)
    assert size(n, 2 * ns) > nb
    lw = torch.randn(n, device=DEV)
    idx = torch.empty(ns, dtype=torch.int64, device=DEV)
    ws = torch.empty(nb + 512, dtype=torch.uint8, device=DEV)
    base = (ws.data_ptr() + 255) & ~255
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda n_=n, ns_=ns, order=0, w=base, wb=nb, lw_=lw.data_ptr(), out=idx.data_ptr(): \
        lib.fabhip_resample_stratified(lw_, n_, 7, ns_, order, out, w, wb, st)      # noqa: E731
    EINVAL, ENOSPC = -1, -4
    assert call(n_=0) == EINVAL and call(ns_=0) == EINVAL and call(ns_=(1 << 31) - 2) == EINVAL
    assert call(order=2) == EINVAL and call(order=-1) == EINVAL
    assert call(w=base + 16) == EINVAL
    assert call(lw_=None) == EINVAL and call(out=None) == EINVAL and call(w=None) == EINVAL
    assert call(wb=nb - 1) == ENOSPC
    assert call() == 0 and call(order=1) == 0
    torch.cuda.synchronize()
    want = spec.stratified(lw.cpu().numpy(), ns, 7, "shuffled")
    np.testing.assert_array_equal(idx.cpu().numpy(), want)
