"""Specification of the seeded stratified resampler (`fabhip_resample_stratified`, and `resample_method="stratified"` of the SMC
mode) as a small CPU program - TEST INFRASTRUCTURE, never imported by the product.  The definition is the project's own; the
device follows it bit for bit and include/fabhip.h restates it.  It composes oracle.numerical (fixed-point CDF, stratum map)
with the counter hash and the keyed permutation of tests/resample_stream_spec.py.

Stratified resampling draws ONE independent uniform per stratum (systematic resampling: one for all of them).  For float32
log_w [n], ns >= 1 draws and a 64-bit seed:

1. C = fixed_point_cdf(log_w), total = C[-1].  total == 0: every index is n - 1 (the rule of the other fixed-point resamplers).
2. F = 62 - bit_length(total), S = (total << F) // ns: systematic_strata(total, ns, 0.0)[:2].
3. h_k = stream_hash(seed, k), k = 0 .. ns - 1 (the splitmix64 finaliser on the stratum number), and
       U_k = (h_k * S) >> 64        the high half of the 128-bit product, an integer in [0, S - 1].
4. t_k = (k S + U_k) >> F, idx_k = first j with C[j] > t_k.  The thresholds are sorted, so the indices are non-decreasing.
5. order "sorted" returns idx, order "shuffled" out[k] = idx[pi(k)], pi = resample_stream_spec.permutation(ns, seed).

Limits: n >= 1, 1 <= ns <= MAX_SAMPLES = 2^31 - 3.  k S + U_k < ns S <= total 2^F < 2^62: 64-bit arithmetic never overflows.

The inverse the device evaluates per CDF value c (closed_form_K): with B = c << F and q = min(B // S, ns),
       K(c) = #{k : t_k < c} = q + [q < ns and q S + U_q < B]
(t_k < c  <=>  k S + U_k < B; the strata below q lie entirely below B, those above q entirely at or above it): item j owns the
strata [K(C[j-1]), K(C[j])).

Inside the SMC mode (decide): the decision of tests/smc_spec.py, unchanged; the ancestors are steps 2 - 4 with ns = n0 and the
seed the 64 bits of the float64 uniform u_j of that transition read as an unsigned integer.
"""
import numpy as np

import smc_spec
from oracle.numerical import fixed_point_cdf, systematic_strata
from resample_stream_spec import ORDERS, permutation, stream_hash

MAX_SAMPLES = (1 << 31) - 3
_M32 = np.uint64(0xFFFFFFFF)


def mulhi64(a: np.ndarray, b: int) -> np.ndarray:
    """(a * b) >> 64 for uint64 a and a scalar b < 2^64, from 32-bit halves."""
    a = np.asarray(a, dtype=np.uint64)
    b = np.uint64(int(b))
    a0, a1, b0, b1 = a & _M32, a >> np.uint64(32), b & _M32, b >> np.uint64(32)
    with np.errstate(over="ignore"):
        p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
        mid = (p00 >> np.uint64(32)) + (p01 & _M32) + (p10 & _M32)
        return p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + (mid >> np.uint64(32))


def strata(total: int, ns: int):
    """(F, S) of point 2."""
    assert total > 0 and 1 <= ns <= MAX_SAMPLES
    F, S, _ = systematic_strata(total, ns, 0.0)
    return F, S


def offsets(seed: int, k, S: int) -> np.ndarray:
    """U_k of point 3 (uint64) for an array of stratum numbers."""
    return mulhi64(stream_hash(seed, k), S)


def thresholds(total: int, ns: int, seed: int) -> np.ndarray:
    F, S = strata(total, ns)
    k = np.arange(ns, dtype=np.uint64)
    return (k * np.uint64(S) + offsets(seed, k, S)) >> np.uint64(F)


def indices_from_cdf(C: np.ndarray, ns: int, seed: int) -> np.ndarray:
    total = int(C[-1])
    if total == 0:
        return np.full(ns, len(C) - 1, dtype=np.int64)
    return np.searchsorted(C, thresholds(total, ns, seed), side="right").astype(np.int64)


def sorted_indices(log_w: np.ndarray, ns: int, seed: int) -> np.ndarray:
    return indices_from_cdf(fixed_point_cdf(np.asarray(log_w, dtype=np.float32)), ns, seed)


def stratified(log_w: np.ndarray, ns: int = None, seed: int = 0, order: str = "sorted") -> np.ndarray:
    log_w = np.asarray(log_w, dtype=np.float32)
    ns = len(log_w) if ns is None else int(ns)
    idx = sorted_indices(log_w, ns, seed)
    if ORDERS[order] == 0:
        return idx
    return idx[permutation(ns, seed)]


def closed_form_K(C: np.ndarray, ns: int, seed: int) -> np.ndarray:
    """K(C[j]) for every j (int64): the number of strata whose threshold lies below C[j]."""
    C = np.asarray(C, dtype=np.uint64)
    F, S = strata(int(C[-1]), ns)
    B = C << np.uint64(F)
    q = np.minimum(B // np.uint64(S), np.uint64(ns))
    qh = np.minimum(q, np.uint64(ns - 1))                      # (the hash of a stratum that exists; unused where q == ns)
    below = (q < np.uint64(ns)) & (qh * np.uint64(S) + offsets(seed, qh, S) < B)
    return (q + below.astype(np.uint64)).astype(np.int64)


def seed_of_uniform(u: float) -> int:
    """The SMC mode's seed: the bits of the float64 u, 0 where u is outside [0, 1) (it is then taken as 0.0)."""
    u = np.float64(u)
    if not (u >= 0.0 and u < 1.0):
        return 0
    return int(np.array([u], dtype=np.float64).view(np.uint64)[0])


def decide(log_w, tau: float, u: float) -> smc_spec.Decision:
    """tests/smc_spec.py: decide with the stratified ancestors in place of the systematic ones."""
    d = smc_spec.decide(log_w, tau, u)
    if not d.resampled:
        return d
    lw = np.asarray(log_w, dtype=np.float32)
    return d._replace(ancestors=sorted_indices(lw, lw.shape[0], seed_of_uniform(u)))
