"""Resampling on the GPU — `resample(x_or_point, log_w)` of fab/sampling_methods/base.py:121-124
(multinomial through torch.multinomial in the reference) plus a systematic resampler.

* `resample(..., method="multinomial")`: scalable fixed-point CDF (single-pass decoupled-look-back
  scan) + two-level binary search + vectorised row gather; uniforms are float64 draws from torch's
  device generator.
* `resample(..., method="multinomial_stream", seed=s)`: seeded streaming multinomial - the sorted draws are generated on
  the fly from exponential spacings (a counter-based hash of the seed) and merged with the CDF; no tensor of uniforms.
* `resample(..., method="stratified", seed=s)`: seeded stratified resampling - one hashed uniform per stratum (unbiased, every
  count within two of its expectation, variance never above multinomial's whatever the order of the particles); the systematic
  resampler's streaming emitter, no CDF and no tensor of uniforms in memory.
* `multinomial_torch_compat(probs, u)`: bit-exact restatement of torch's CPU multinomial given the
  probabilities and the float64 uniforms it consumed (parity with the reference's RNG path).
"""
from typing import Union

import torch

from . import _ops
from .point import Point


def multinomial_indices(log_w: torch.Tensor, n_samples: int = None, u: torch.Tensor = None) -> torch.Tensor:
    _ops.require_device(log_w, "log_w")
    lw = log_w.detach().contiguous().float()
    ns = lw.shape[0] if n_samples is None else int(n_samples)
    if u is None:
        u = torch.rand(ns, dtype=torch.float64, device=lw.device)
    return _ops.load().resample_multinomial(lw, u.contiguous().double())


def systematic_indices(log_w: torch.Tensor, u0: float = None, n_samples: int = None) -> torch.Tensor:
    _ops.require_device(log_w, "log_w")
    lw = log_w.detach().contiguous().float()
    ns = lw.shape[0] if n_samples is None else int(n_samples)
    if u0 is None:
        u0 = float(torch.rand((), dtype=torch.float64))
    return _ops.load().resample_systematic(lw, float(u0), ns)


STREAM_ORDERS = {"sorted": 0, "shuffled": 1}          # FABHIP_ORDER_*


def _seed64(seed) -> int:
    """The 64 bits of `seed` as the signed integer the ops take; None: 64 bits from torch's CPU generator."""
    if seed is None:
        seed = int(torch.randint(-(1 << 63), (1 << 63) - 1, (), dtype=torch.int64))
    seed = int(seed) & ((1 << 64) - 1)
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def stratified_indices(log_w: torch.Tensor, n_samples: int = None, seed: int = None, order: str = "sorted") -> torch.Tensor:
    """Stratified resampling indices from `(log_w, seed)` alone (include/fabhip.h: fabhip_resample_stratified): stratum k of
    the `n_samples` equal strata of the fixed-point CDF draws its own offset, a hash of `(seed, k)`.  `order="sorted"`:
    non-decreasing indices; `order="shuffled"`: the same indices in the seeded random order of `multinomial_stream_indices`.
    `seed=None` draws 64 bits from torch's CPU generator; the same `(log_w, n_samples, seed, order)` gives the same indices on
    any device.  1 <= n_samples <= 2^31 - 3."""
    _ops.require_device(log_w, "log_w")
    if order not in STREAM_ORDERS:
        raise _ops.FabhipError(f"order must be 'sorted' or 'shuffled' (got {order!r})")
    lw = log_w.detach().contiguous().float()
    ns = lw.shape[0] if n_samples is None else int(n_samples)
    return _ops.load().resample_stratified(lw, _seed64(seed), ns, STREAM_ORDERS[order])


def multinomial_stream_indices(log_w: torch.Tensor, n_samples: int = None, seed: int = None,
                               order: str = "sorted") -> torch.Tensor:
    """Multinomial resampling indices from `(log_w, seed)` alone (include/fabhip.h: fabhip_resample_multinomial_stream).
    `order="sorted"`: non-decreasing indices (what a row gather needs, like `systematic_indices`); `order="shuffled"`: the same
    indices in a seeded random order - an exchangeable sample, as `torch.multinomial` gives.  `seed=None` draws 64 bits from
    torch's CPU generator; the same `(log_w, n_samples, seed, order)` gives the same indices on any device."""
    _ops.require_device(log_w, "log_w")
    if order not in STREAM_ORDERS:
        raise _ops.FabhipError(f"order must be 'sorted' or 'shuffled' (got {order!r})")
    lw = log_w.detach().contiguous().float()
    ns = lw.shape[0] if n_samples is None else int(n_samples)
    return _ops.load().resample_multinomial_stream(lw, _seed64(seed), ns, STREAM_ORDERS[order])


def multinomial_torch_compat(probs: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    _ops.require_device(probs, "probs")
    return _ops.load().multinomial_torch(probs.detach().contiguous().float(), u.contiguous().double())


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    _ops.require_device(src, "src")
    return _ops.load().gather_rows(src.contiguous().float(), idx.contiguous())


def resample(x_or_point: Union[Point, torch.Tensor], log_w: torch.Tensor, method: str = "multinomial", seed: int = None):
    """Resample points according to the log weights (same call shape as the reference).  `seed` belongs to
    `method="multinomial_stream"` and `method="stratified"` (the other methods draw from torch's generators)."""
    if method == "multinomial_stream":
        idx = multinomial_stream_indices(log_w, seed=seed)
    elif method == "stratified":
        idx = stratified_indices(log_w, seed=seed)
    else:
        idx = multinomial_indices(log_w) if method == "multinomial" else systematic_indices(log_w)
    if isinstance(x_or_point, Point):
        p = x_or_point
        g = lambda t: None if t is None else gather_rows(t, idx)
        return Point(g(p.x), g(p.log_q), g(p.log_p), g(p.grad_log_q), g(p.grad_log_p))
    return gather_rows(x_or_point, idx)
