"""Specification of the seeded streaming multinomial resampler (`fabhip_resample_multinomial_stream`) as a small CPU program -
TEST INFRASTRUCTURE, never imported by the product.  The definition is the project's own (like the systematic resampler's,
oracle/numerical.py: systematic_fixed); the device follows it bit for bit and include/fabhip.h restates the constants.

Multinomial resampling needs ns iid uniforms; only their ORDER STATISTICS decide which particle owns how many draws, and those
can be generated directly in sorted order: with E_0 .. E_ns iid exponential, U_(k) = (E_0 + .. + E_k) / (E_0 + .. + E_ns),
k = 0 .. ns - 1, are distributed as the sorted values of ns iid uniforms.  Sorted thresholds make resampling a merge of two
sorted sequences.

1. W = oracle.numerical.fixed_point_weights(log_w) (uint64, non-finite rows weigh 0), C = cumsum(W), total = C[-1].
   total == 0: every index is n - 1.
2. Spacing i, 0 <= i <= ns, from the 64-bit seed - integer operations modulo 2^64 (the splitmix64 finaliser on a counter):
       z = seed + (i + 1) * 0x9E3779B97F4A7C15
       z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  r_i = z ^ (z >> 31)
   y = (r_i >> 32) | 1 (odd, 1 <= y < 2^32), lz = count of leading zeros of the 32-bit y, mant = ((y << lz) mod 2^32) >> 8
   (24 bits, top bit set).  The uniform is u_i = f * 2^-(lz + 1) with f = mant 2^-23 in [1, 2): strictly inside (0, 1), a
   float32-like grid that gets finer towards 0.
   -ln(u_i) = K ln 2 - ln(g) with red = (f >= 1.41421354f), g = red ? f / 2 : f (exact), K = lz + 1 - red.
   t = g - 1 (exact, -0.2929 <= t < 0.4143) and ln(1 + t) ~ p(t) = t (c0 + t (c1 + .. + t c8)) evaluated by Horner's rule in
   float32, every multiply and every add individually rounded (LOG_C below, highest coefficient first).
       e_i = max(1, K * LN2_FIX - int(rint(p * 2^28)))       LN2_FIX = 186065279 = round(ln 2 * 2^28)
   an unsigned fixed-point number with FRAC_BITS = 28 fractional bits.
   Error: |e_i 2^-28 + ln(u_i)| <= 1.3e-7.  The polynomial part |p(t) - ln(1 + t)| <= 5.2e-8 is MEASURED OVER ALL 2^23 values of
   f (the test repeats that exhaustive check), rint adds 2^-29, K <= 32 times |LN2_FIX 2^-28 - ln 2| = 1.83e-9 adds 5.9e-8,
   and the clamp at 1 only acts where -ln(u_i) < 1.2e-7.
   e_i <= 32 * LN2_FIX < 2^33, so G_ns < 2^62 for ns + 1 <= 2^29:  MAX_SAMPLES = 2^29 - 1, larger ns is refused.
3. G_k = e_0 + .. + e_k (exact integers).  Sorted draw k, 0 <= k < ns:  idx_k = first j with C_j * G_ns > G_k * total
   (128-bit products), equivalently first j with C_j > floor(G_k * total / G_ns).  e_ns >= 1 keeps G_k < G_ns.
4. order "sorted" returns idx; order "shuffled" returns out[k] = idx[pi(k)], pi a keyed bijection of [0, ns): four Feistel
   rounds on the next power of two >= max(ns, 4) with cycle walking back into range (topk.hip: k_random_order), round keys
   key_j = low 32 bits of r_i for i = 2^40 + j (beyond every legal spacing index), round function the murmur3 finaliser.
"""
import numpy as np

from oracle.numerical import FIX_BITS, fixed_point_weights  # noqa: F401  (FIX_BITS: the weights' fractional bits)

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MIX1, MIX2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
FRAC_BITS = 28
LN2_FIX = 186065279
SQRT2_F = np.float32(1.41421354)
LOG_C = [np.float32(c) for c in (0.08743945509195328, -0.14377330243587494, 0.14949095249176025, -0.16560696065425873,
                                 0.19956977665424347, -0.2500215470790863, 0.3333418369293213, -0.49999988079071045, 1.0)]
MAX_SAMPLES = (1 << 29) - 1
KEY_BASE = 1 << 40
LOG_BOUND = 1.3e-7
ORDERS = {"sorted": 0, "shuffled": 1}


def stream_hash(seed: int, i) -> np.ndarray:
    """r_i of point 2 for an array of counters (uint64 arithmetic wraps modulo 2^64)."""
    i = np.asarray(i, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & MASK64) + (i + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
    return z ^ (z >> np.uint64(31))


def _log_parts(y: np.ndarray):
    """(K, g) of the odd 32-bit integers y: -ln(u) = K ln 2 - ln g, g a float32 in [0.7071, 1.4143)."""
    y = np.asarray(y, dtype=np.uint64)
    nbits = np.zeros(y.shape, dtype=np.int64)                 # bit length of y (1 .. 32), by integer comparisons
    for b in range(32):
        nbits += (y >= np.uint64(1 << b)).astype(np.int64)
    lz = 32 - nbits
    mant = ((y << lz.astype(np.uint64)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)
    f = (mant.astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    red = f >= SQRT2_F
    g = np.where(red, (f * np.float32(0.5)).astype(np.float32), f).astype(np.float32)
    return lz + 1 - red.astype(np.int64), g


def log_poly(g: np.ndarray) -> np.ndarray:
    """p(t) ~ ln(g), t = g - 1: float32 Horner, each operation rounded."""
    t = (np.asarray(g, np.float32) - np.float32(1)).astype(np.float32)
    p = np.full_like(t, LOG_C[0])
    for c in LOG_C[1:]:
        p = (p * t).astype(np.float32)
        p = (p + c).astype(np.float32)
    return (p * t).astype(np.float32)


def neg_log_fixed(r: np.ndarray) -> np.ndarray:
    """e of point 2 (uint64, >= 1) for hashed words r."""
    y = (np.asarray(r, np.uint64) >> np.uint64(32)) | np.uint64(1)
    K, g = _log_parts(y)
    lnf = np.rint((log_poly(g) * np.float32(2.0 ** FRAC_BITS)).astype(np.float32)).astype(np.int64)
    return np.maximum(K * LN2_FIX - lnf, 1).astype(np.uint64)


def uniform_of(r: np.ndarray) -> np.ndarray:
    """u of point 2 as float64 (exact): what neg_log_fixed approximates the -ln of."""
    y = (np.asarray(r, np.uint64) >> np.uint64(32)) | np.uint64(1)
    K, g = _log_parts(y)
    return np.ldexp(g.astype(np.float64), (-K).astype(np.int64))


def spacings(seed: int, ns: int) -> np.ndarray:
    """e_0 .. e_ns (uint64)."""
    return neg_log_fixed(stream_hash(seed, np.arange(ns + 1, dtype=np.uint64)))


def floor_muldiv(G: np.ndarray, total: int, Gn: int) -> np.ndarray:
    """floor(G * total / Gn) exactly, G <= Gn < 2^62, total < 2^62.  Python integers define it; below total = 2^50 a float64
    estimate (off by at most one) with one exact correction on the wrapped 64-bit remainder gives the same, vectorised."""
    G = np.asarray(G, dtype=np.uint64)
    if total >= (1 << 50):
        return np.array([(int(g) * total) // Gn for g in G], dtype=np.uint64)
    q = np.floor(G.astype(np.float64) * np.float64(total) / np.float64(Gn)).astype(np.uint64)
    with np.errstate(over="ignore"):
        rem = (G * np.uint64(total) - q * np.uint64(Gn)).view(np.int64)      # |G total - q Gn| < 2 Gn < 2^63
    q = q - (rem < 0).astype(np.uint64)
    q = q + (rem >= np.int64(Gn)).astype(np.uint64)
    return q


def thresholds(log_w: np.ndarray, ns: int, seed: int, positions=None):
    """(C, t): the fixed-point CDF and t_k = floor(G_k total / G_ns) of the sorted draws `positions` (default: all)."""
    assert 1 <= ns <= MAX_SAMPLES
    C = np.cumsum(fixed_point_weights(log_w), dtype=np.uint64)
    G = np.cumsum(spacings(seed, ns), dtype=np.uint64)
    Gn, total = int(G[-1]), int(C[-1])
    assert Gn < (1 << 62)
    Gk = G[:ns] if positions is None else G[np.asarray(positions, dtype=np.int64)]
    return C, (floor_muldiv(Gk, total, Gn) if total > 0 else None)


def sorted_indices(log_w: np.ndarray, ns: int, seed: int, positions=None) -> np.ndarray:
    C, t = thresholds(log_w, ns, seed, positions)
    if t is None:
        return np.full(ns if positions is None else len(positions), len(C) - 1, dtype=np.int64)
    return np.searchsorted(C, t, side="right").astype(np.int64)


def _mix32(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def permutation(ns: int, seed: int) -> np.ndarray:
    """pi(0 .. ns - 1) of point 4."""
    bits = 2
    while (1 << bits) < ns:
        bits += 1
    lb = bits >> 1
    rb = bits - lb
    lm, rm = np.uint64((1 << lb) - 1), np.uint64((1 << rb) - 1)
    keys = stream_hash(seed, KEY_BASE + np.arange(4, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    v = np.arange(ns, dtype=np.uint64)
    todo = np.ones(ns, dtype=bool)
    while todo.any():
        w = v[todo]
        l, r = (w >> np.uint64(rb)) & lm, w & rm
        for j in range(4):
            if j & 1:
                r = r ^ (_mix32(l ^ keys[j]) & rm)
            else:
                l = l ^ (_mix32(r ^ keys[j]) & lm)
        w = (l << np.uint64(rb)) | r
        v[todo] = w
        todo[todo] = w >= np.uint64(ns)
    return v.astype(np.int64)


def multinomial_stream(log_w: np.ndarray, ns: int = None, seed: int = 0, order: str = "sorted") -> np.ndarray:
    log_w = np.asarray(log_w, dtype=np.float32)
    ns = len(log_w) if ns is None else int(ns)
    idx = sorted_indices(log_w, ns, seed)
    if ORDERS[order] == 0:
        return idx
    return idx[permutation(ns, seed)]
