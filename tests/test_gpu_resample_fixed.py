"""GPU tests of the fixed-point resamplers behind `resample` (fabhip_fixed_cdf, fabhip_resample_multinomial,
fabhip_resample_systematic on both of its paths, fabhip_gather_rows; csrc/resample_scan.hip, resample_emit.hip and
reduce_kernels.hip) against oracle/numerical.py on the
cases of tests/resample_fixed_cases.py: sizes around every lane-row / node / tile / workgroup boundary, more and fewer draws than
weights, degenerate weights (test_resample_fixed_cases.py holds each case to the branch it is listed for).  Integer work with an
exact statement: every comparison is bit for bit.

The samplers are driven through the C ABI with ONE caller-owned workspace for the whole file, pre-filled with 0xA5 bytes and never
cleared, and an index buffer pre-filled with -1: a word the kernels leave unwritten, or read before writing, shows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import resample_fixed_cases as rc

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _lib, _ops     # noqa: E402

DEV = "cuda"
MAX_N = 70_001


@functools.lru_cache(maxsize=None)
def _workspace():
    lib = _lib.load()
    nb = int(lib.fabhip_resample_workspace_bytes(MAX_N))
    buf = torch.full((nb + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    skip = -buf.data_ptr() % 256
    return buf, skip, nb


def _ws_args(n):
    buf, skip, nb = _workspace()
    assert _lib.load().fabhip_resample_workspace_bytes(n) <= nb
    return C.c_void_p(buf.data_ptr() + skip), nb


@functools.lru_cache(maxsize=None)
def _device_log_w(name):
    """ONE device copy of a case's log_w (the unaligned case: inside a buffer, one float behind its 16-byte aligned start)."""
    case = rc.get_case(name)
    lw = torch.tensor(case.log_w).to(DEV)
    if case.unaligned:
        buf = torch.empty(len(case.log_w) + 1, device=DEV)
        buf[1:] = lw
        lw = buf[1:]
        assert lw.data_ptr() % 16 != 0
    else:
        assert lw.data_ptr() % 16 == 0
    assert lw.is_contiguous() and lw.dtype == torch.float32
    return lw


def _systematic(lw_d, u0, ns, variant):
    idx = torch.full((ns,), -1, dtype=torch.int64, device=DEV)
    ws, nb = _ws_args(lw_d.numel())
    with _ops.option(_ops.OPT_SYSTEMATIC_VARIANT, variant):        # restored on exit, whatever the call does
        rc_ = _lib.load().fabhip_resample_systematic(_lib.ptr(lw_d), lw_d.numel(), float(u0), ns, _lib.ptr(idx), ws, nb,
                                                      _lib.stream_ptr())
    _lib.check(rc_, "resample_systematic")
    return idx.cpu().numpy()


def _multinomial(lw_d, u):
    idx = torch.full((len(u),), -1, dtype=torch.int64, device=DEV)
    u_d = torch.tensor(u, dtype=torch.float64).to(DEV)
    ws, nb = _ws_args(lw_d.numel())
    _lib.check(_lib.load().fabhip_resample_multinomial(_lib.ptr(lw_d), lw_d.numel(), _lib.ptr(u_d), len(u), _lib.ptr(idx), ws, nb,
                                                       _lib.stream_ptr()), "resample_multinomial")
    return idx.cpu().numpy()


def _check_systematic(name):
    case = rc.get_case(name)
    lw_d = _device_log_w(name)
    default = _ops.load().get_option(_ops.OPT_SYSTEMATIC_VARIANT)
    for ns in case.ns:
        for u0 in case.u0:
            want = rc.expected_systematic(case, ns, u0)
            fused = _systematic(lw_d, u0, ns, 1)
            np.testing.assert_array_equal(fused, want, err_msg=f"{name} ns={ns} u0={u0!r} fused path")
            hbm = _systematic(lw_d, u0, ns, 0)
            np.testing.assert_array_equal(hbm, want, err_msg=f"{name} ns={ns} u0={u0!r} CDF-in-HBM path")
            np.testing.assert_array_equal(fused, hbm)
    assert _ops.load().get_option(_ops.OPT_SYSTEMATIC_VARIANT) == default


# ---- CDF ----
@pytest.mark.parametrize("name", rc.EDGE_NAMES + ("heavy_tail", "dead_middle", "nan_inf", "all_dead", "unaligned"))
def test_fixed_cdf_bit_exact_vs_oracle(name):
    """The look-back scan's n CDF words (default scan, FABHIP_OPT_SCAN_VARIANT = 3) against fixed_point_cdf; a second call that
    reuses the maximum the first one left in the workspace rewrites the same words."""
    lib = _lib.load()
    assert _ops.load().get_option(_ops.OPT_SCAN_VARIANT) == 3
    case = rc.get_case(name)
    n = len(case.log_w)
    lw_d = _device_log_w(name)
    buf, skip, _ = _workspace()
    ws, nb = _ws_args(n)
    want = rc.expected_cdf(case)
    for reuse_max in (0, 1):
        out = C.c_void_p()
        _lib.check(lib.fabhip_fixed_cdf(_lib.ptr(lw_d), n, reuse_max, C.cast(C.pointer(out), C.c_void_p), ws, nb,
                                        _lib.stream_ptr()), "fixed_cdf")
        off = out.value - buf.data_ptr()
        assert skip <= off and off % 8 == 0 and off + 8 * n <= buf.numel()
        words = buf[off: off + 8 * n].view(torch.int64)
        got = words.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(got, want, err_msg=f"{name} reuse_max={reuse_max}")
        words.fill_(-1)                                      # the second pass has every word to write again


# ---- systematic: fused emitter and CDF-in-HBM path ----
@pytest.mark.parametrize("name", rc.EDGE_NAMES)
def test_systematic_edge_sizes_bit_exact_vs_oracle(name):
    _check_systematic(name)


@pytest.mark.parametrize("name", rc.SPECIAL_NAMES)
def test_systematic_special_weights_bit_exact_vs_oracle(name):
    _check_systematic(name)


def test_systematic_keeps_no_state_between_calls():
    """The same call before and after calls of other sizes on the same stream and workspace: the giant-run list, its counter and
    the stratum map live in scratch that the calls in between overwrite."""
    ht, lf, mx = rc.get_case("heavy_tail"), rc.get_case("list_full"), rc.get_case("mixed")
    ns = ht.ns[-1]
    want = rc.expected_systematic(ht, ns, 0.37)
    for variant in (1, 0):
        np.testing.assert_array_equal(_systematic(_device_log_w("heavy_tail"), 0.37, ns, variant), want)
        np.testing.assert_array_equal(_systematic(_device_log_w("list_full"), 0.37, lf.ns[0], variant),
                                      rc.expected_systematic(lf, lf.ns[0], 0.37))
        np.testing.assert_array_equal(_systematic(_device_log_w("mixed"), 0.0, mx.ns[-1], variant),
                                      rc.expected_systematic(mx, mx.ns[-1], 0.0))
        np.testing.assert_array_equal(_systematic(_device_log_w("heavy_tail"), 0.37, ns, variant), want)
    # and through the op, which takes its scratch from the caching allocator
    a = fa.systematic_indices(_device_log_w("heavy_tail"), u0=0.37, n_samples=ns)
    fa.systematic_indices(_device_log_w("list_full"), u0=0.37, n_samples=lf.ns[0])
    b = fa.systematic_indices(_device_log_w("heavy_tail"), u0=0.37, n_samples=ns)
    np.testing.assert_array_equal(a.cpu().numpy(), want)
    np.testing.assert_array_equal(b.cpu().numpy(), want)


# ---- multinomial ----
@pytest.mark.parametrize("name", rc.ALL_NAMES)
def test_multinomial_bit_exact_vs_oracle(name):
    """Draw counts around the wave's 64 (a wave-uniform trip count with a ragged tail), u = 0 and the float64 below 1, thresholds
    one below and on the CDF steps at tile / 256-node / 16-node ends and at the last live index (rc.multinomial_u)."""
    case = rc.get_case(name)
    n = len(case.log_w)
    lw_d = _device_log_w(name)
    for ns in (1, 63, 64, 65, n, 3 * n + 5):
        u = rc.multinomial_u(case, ns)
        np.testing.assert_array_equal(_multinomial(lw_d, u), rc.expected_multinomial(case, u), err_msg=f"{name} ns={ns}")


# ---- gather_rows ----
@pytest.mark.parametrize("name", ["heavy_tail", "all_equal"])
def test_gather_rows_bit_exact(name):
    case = rc.get_case(name)
    n = len(case.log_w)
    idx = torch.tensor(rc.expected_systematic(case, n, 0.37)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(n)
    for row_len in (1, 3, 4, 6, 32, 33):
        src = torch.randn(n, row_len, device=DEV, generator=g)
        got = fa.gather_rows(src, idx)
        assert got.shape == (n, row_len)
        assert torch.equal(got.view(torch.int32), src[idx].view(torch.int32)), f"{name} row_len={row_len}"
    # rows of four floats whose base is one float off 16-byte alignment: the scalar path although row_len % 4 == 0
    buf = torch.randn(4 * n + 1, device=DEV, generator=g)
    src = buf[1:].view(n, 4)
    assert src.data_ptr() % 16 != 0 and src.is_contiguous()
    assert torch.equal(fa.gather_rows(src, idx).view(torch.int32), src[idx].view(torch.int32))
    flat = fa.gather_rows(src[:, 0].contiguous(), idx)            # a 1-D source: rows of one float
    assert torch.equal(flat, src[:, 0][idx])


# ---- resample ----
def test_resample_point_with_one_survivor():
    """ESS collapse as AIS hands it over: every field of the resampled Point is the survivor's row."""
    case = rc.get_case("one_survivor")
    n, D, s = len(case.log_w), 6, 43210
    g = torch.Generator(device=DEV).manual_seed(1)
    p = fa.Point(torch.randn(n, D, device=DEV, generator=g), torch.randn(n, device=DEV, generator=g),
                 torch.randn(n, device=DEV, generator=g), torch.randn(n, D, device=DEV, generator=g),
                 torch.randn(n, D, device=DEV, generator=g))
    lw_d = _device_log_w("one_survivor")
    for method in ("systematic", "multinomial"):
        r = fa.resample(p, lw_d, method=method)
        for got, src in ((r.x, p.x), (r.log_q, p.log_q), (r.log_p, p.log_p), (r.grad_log_q, p.grad_log_q),
                         (r.grad_log_p, p.grad_log_p)):
            assert got.shape == src.shape
            assert torch.equal(got, src[s].expand_as(src)), method
    assert torch.equal(fa.resample(p.x, lw_d, method="systematic"), p.x[s].expand_as(p.x))
