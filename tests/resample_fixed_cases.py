"""Named inputs of the fixed-point resamplers (fabhip_resample_multinomial, csrc/resample_scan.hip; fabhip_resample_systematic,
csrc/resample_emit.hip and, for its scan + search path, resample_scan.hip) shared by test_resample_fixed_cases.py (CPU: every
case reaches the device branch it is listed for, judged from the oracle's output alone) and test_gpu_resample_fixed.py (GPU: bit-exact against oracle/numerical.py).  No test functions here.

A case is (name, float32 log_w from a seeded np.random.default_rng, the n_samples to draw, the u0 to draw them with).  The
constants below restate the kernel constants that decide which branch a wave takes; a change on either side shows up in the CPU
file as a branch that is no longer reached."""
import functools
from collections import namedtuple

import numpy as np

from oracle import numerical as onum

# ---- kernel constants that decide a branch (EM_*: csrc/resample_emit.hip; SCAN_* / SYS_*: csrc/resample_scan.hip) ----
EM_WAVE_ITEMS = 1024        # constexpr int EM_WAVE_ITEMS: weights per wave of k_emit_systematic
EM_NW = 4                   # constexpr int EM_NW: waves per workgroup (EM_BLOCK = EM_WAVE_ITEMS * EM_NW)
EM_WIN = 1536               # constexpr int EM_WIN: strata per marker window
EM_GIANT = 32768            # constexpr int EM_GIANT: runs at least this long are published to k_emit_fill_runs
EM_F64_STRATA = 1 << 20     # `if (T < (1 << 20))` in k_emit_systematic: from here on the float64 per-item estimate
SCAN_TILE = 4096            # constexpr int SCAN_TILE: weights per search tile (one tile_inc word each)
SYS_CHUNK = 4096            # constexpr int SYS_CHUNK: samples per workgroup of k_sample_systematic
SYS_MAX_SPAN = 8            # constexpr int SYS_MAX_SPAN: chunks over more tiles take the global search


def giant_capacity(n: int, ns: int) -> int:
    """`giant_cap` of fabhip_resample_systematic: the words the wave sums, block sums, prefixes, stratum map and run counter
    leave of the n-word CDF region, three per run, at most ns / EM_GIANT + 1."""
    nwt = (n + EM_WAVE_ITEMS - 1) // EM_WAVE_ITEMS
    nbk = (n + EM_WAVE_ITEMS * EM_NW - 1) // (EM_WAVE_ITEMS * EM_NW)
    left = n - (nwt + 2 * nbk + 5)
    cap = -((-left) // 3) if left < 0 else left // 3          # C++ division truncates towards zero
    return min(max(cap, 0), ns // EM_GIANT + 1)


# ---- a stratum threshold ON a CDF value, and the float64 estimate of the inverse stratum map there ----
def on_step_u0(total: int, ns: int, c: int):
    """u0 with (c << F) - U a multiple of S: the threshold t_m = (m S + U) >> F of some stratum m is exactly c (None when no
    float64 u0 gives that U)."""
    F, S, _ = onum.systematic_strata(total, ns, 0.0)
    U = (int(c) << F) % S
    u0 = (U + 0.5) / S
    if not u0 < 1.0 or onum.systematic_strata(total, ns, u0)[2] != U:
        return None
    return u0


def f64_estimate(total: int, ns: int, u0: float, c0: int, d: int):
    """(estimate, exact) of K(c0 + d) = ceil((((c0 + d) << F) - U) / S): `stratum_rel`'s float64 expression
    ceil(((double)d * 2^F + (double)((c0 << F) - U)) * (1.0 / (double)S)) before its integer correction step, and the integer."""
    F, S, U = onum.systematic_strata(total, ns, u0)
    B0 = int(c0) << F
    num0 = float(B0 - U) if B0 >= U else -float(U - B0)
    y = (float(int(d)) * float(1 << F) + num0) * (1.0 / float(S))
    X = ((int(c0) + int(d)) << F) - U
    return int(np.ceil(y)), -((-X) // S)


def overshooting_u0(total: int, ns: int, pairs):
    """(u0, ns, c0, d) of the first (c0, d) of `pairs` whose on-step u0 makes the float64 estimate exceed the exact K: the
    `--k` branch of the correction step decides the result there."""
    for c0, d in pairs:
        if not 0 < c0 + d < total:
            continue
        u0 = on_step_u0(total, ns, c0 + d)
        if u0 is not None:
            est, exact = f64_estimate(total, ns, u0, c0, d)
            if est > exact:
                return u0, ns, c0, d
    return None


# ---- the cases ----
Case = namedtuple("Case", "name log_w ns u0 unaligned on_step")      # on_step: (ns, c0, d) behind the constructed u0[3], or None

EDGE_N = (1, 2, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 65537)
U0 = (0.37, 0.0, float(np.nextafter(1.0, 0.0)))
SPECIAL_N = 70_001
# what each special case is for (tests/README.md repeats it)
SPECIAL = {
    "one_survivor": "one run holds every stratum: published, every window skipped; float64 estimate at the larger n_samples",
    "heavy_tail": "two indices share everything: giant runs that start / end inside a window; chunks over more than 8 tiles",
    "mixed": "a published giant run beside thousands of ordinary runs; a wave's first threshold ON its CDF start, estimate one high",
    "hot_wave": "one wave owns >= 32768 strata without a giant run; at 16n + 3 the float64 estimate on ~1000 distinct runs, one "
                "of them with a threshold ON its CDF value and the estimate one high",
    "few_weights_many_draws": "a ragged last wave that owns every stratum, float64 estimate",
    "list_full": "more giant runs than the list holds (capacity 1): the rest stay with their wave",
    "no_list": "capacity 0: no run is published, the fill kernel is not launched",
    "dead_middle": "a long dead stretch: chunks over more than 8 tiles, waves without a stratum",
    "all_equal": "every weight 2^36: thresholds on CDF steps, the largest total",
    "all_dead": "total 0: every index n - 1",
    "nan_inf": "NaN, +inf and -inf rows weigh 0",
    "unaligned": "a log_w pointer off 16-byte alignment: the scalar staging loops",
}


def _seed(name):
    return sum(map(ord, name))


@functools.lru_cache(maxsize=None)
def edge_case(N: int) -> Case:
    rng = np.random.default_rng(4000 + N)
    lw = (rng.standard_normal(N) * 2.5).astype(np.float32)
    if N > 40:
        lw[: N // 9] = -np.inf
        lw[-(N // 11):] = -np.inf
    lw.setflags(write=False)
    return Case(f"edge_{N}", lw, (N, 3 * N + 5, max(1, N // 3), 1, 63, 64, 65), U0, False, None)


@functools.lru_cache(maxsize=None)
def special_case(name: str) -> Case:
    rng = np.random.default_rng(_seed(name))
    n = SPECIAL_N
    if name == "few_weights_many_draws":
        lw, ns = rng.standard_normal(300).astype(np.float32), ((1 << 20) + 5,)
    elif name == "list_full":
        lw, ns = np.full(12, 0.25, np.float32), (480_000,)
    elif name == "no_list":
        lw, ns = np.full(5, 0.25, np.float32), (200_000,)
    else:
        lw, ns = (rng.standard_normal(n) * 2).astype(np.float32), (n,)
        if name == "one_survivor":
            lw[:] = -np.inf; lw[43210] = 0.5
            ns = (n, (1 << 20) + 4097)
        elif name == "heavy_tail":
            lw[12345] = 40.0; lw[60000] = 38.5
            ns = (n, 3 * n + 5, (1 << 21) + 3)
        elif name == "mixed":
            lw[12345] = 12.0; lw[60000] = 11.5
            ns = (n, 3 * n + 5)
        elif name == "hot_wave":
            lw[2048:3072] += 9.0
            ns = (n, 16 * n + 3)
        elif name == "dead_middle":
            lw[10000:55000] = -np.inf
            ns = (n, 9000)
        elif name == "all_equal":
            lw[:] = 1.25
            ns = (n, 3 * n + 5)
        elif name == "all_dead":
            lw[:] = -np.inf
            ns = (n, 77)
        elif name == "nan_inf":
            lw[20000:23000] = np.nan; lw[100:200] = np.inf; lw[-5000:] = -np.inf
        elif name != "unaligned":
            raise KeyError(name)
    lw.setflags(write=False)
    u0, on_step = U0, None
    if name in ("mixed", "unaligned", "hot_wave"):
        # a fourth u0 that puts a stratum threshold exactly ON a CDF value whose float64 estimate of K(C) comes out one too high:
        # the value of a wave's first stratum (mixed, unaligned) / of an item of the hot wave in the float64 branch (hot_wave)
        C = onum.fixed_point_cdf(lw)
        if name == "hot_wave":
            pairs = [(int(C[2047]), int(C[j]) - int(C[2047])) for j in range(2048, 3071)]
        else:
            pairs = [(int(C[j]), 0) for j in range(EM_WAVE_ITEMS - 1, n - 1, EM_WAVE_ITEMS)]
        found = overshooting_u0(int(C[-1]), ns[-1] if name == "hot_wave" else ns[0], pairs)
        if found is not None:
            u0, on_step = U0 + (found[0],), found[1:]
    return Case(name, lw, ns, u0, name == "unaligned", on_step)


def get_case(name: str) -> Case:
    return edge_case(int(name[5:])) if name.startswith("edge_") else special_case(name)


EDGE_NAMES = tuple(f"edge_{N}" for N in EDGE_N)
SPECIAL_NAMES = tuple(SPECIAL)
ALL_NAMES = EDGE_NAMES + SPECIAL_NAMES


# ---- expectations: oracle/numerical.py, plus the all-dead rule of include/fabhip.h (total == 0: every index n - 1) ----
@functools.lru_cache(maxsize=None)
def _cdf(name: str) -> np.ndarray:
    C = onum.fixed_point_cdf(get_case(name).log_w)
    C.setflags(write=False)
    return C


def expected_cdf(case: Case) -> np.ndarray:
    return _cdf(case.name)


def total_of(case: Case) -> int:
    return int(_cdf(case.name)[-1])


def expected_systematic(case: Case, ns: int, u0: float) -> np.ndarray:
    if total_of(case) == 0:
        return np.full(ns, len(case.log_w) - 1, np.int64)
    return onum.systematic_fixed(case.log_w, u0, ns)


def expected_multinomial(case: Case, u: np.ndarray) -> np.ndarray:
    if total_of(case) == 0:
        return np.full(len(u), len(case.log_w) - 1, np.int64)
    return onum.multinomial_fixed(case.log_w, u)


def boundary_items(case: Case, limit: int = 32):
    """Items whose CDF value the multinomial thresholds are put on and beside: the last live item, then the last / first item
    of search tiles, 256-nodes and 16-nodes (the first two, the last two and the one around the middle of each kind)."""
    n = len(case.log_w)
    C = expected_cdf(case)
    live = np.flatnonzero(np.diff(np.concatenate([[0], C.astype(np.int64)])) > 0)
    out = [int(live[-1])] if len(live) else []
    if len(live) > 1:
        out.append(int(live[-2]))
    for b in (SCAN_TILE, 256, 16):
        ends = list(range(b - 1, n, b))
        pick = ends[:2] + ends[-2:] + ends[len(ends) // 2: len(ends) // 2 + 1]
        for e in pick:
            out += [e, e + 1]
    out += [0, n - 1]
    seen, res = set(), []
    for j in out:
        if 0 <= j < n and j not in seen:
            seen.add(j); res.append(j)
    return res[:limit]


def multinomial_u(case: Case, ns: int) -> np.ndarray:
    """float64 draws: seeded uniforms; u[0] = 0, u[1] = the float64 below 1; then, as far as ns reaches, pairs
    (C[j] - 0.5) / total, (C[j] + 0.5) / total for the items of `boundary_items`: thresholds one below and on a CDF step."""
    rng = np.random.default_rng(_seed(case.name) + 7919 * ns)
    u = rng.random(ns)
    top = float(np.nextafter(1.0, 0.0))
    u[0] = 0.0
    if ns > 1:
        u[1] = top
    total = total_of(case)
    if total > 0:
        C = expected_cdf(case)
        extra = []
        for j in boundary_items(case):
            extra += [(float(C[j]) - 0.5) / float(total), (float(C[j]) + 0.5) / float(total)]
        extra = np.clip(np.array(extra, np.float64), 0.0, top)
        m = max(0, min(len(extra), ns - 2))
        u[2:2 + m] = extra[:m]
    return u


# ---- which branches a systematic call takes, from the oracle's output alone ----
def branch_profile(log_w: np.ndarray, ns: int, u0: float) -> dict:
    """Per wave tile of EM_WAVE_ITEMS weights: `strata` owned (the kernel's T), `longest` run, `giants` = runs >= EM_GIANT,
    `distinct` = indices drawn at least once; `capacity` of the giant list; `chunk_span` = the most search tiles one chunk
    of SYS_CHUNK samples touches (k_sample_systematic's tb - ta + 1); `total` of the fixed-point weights."""
    n = len(log_w)
    total = int(onum.fixed_point_cdf(log_w)[-1])
    nw = (n + EM_WAVE_ITEMS - 1) // EM_WAVE_ITEMS
    prof = {"total": total, "capacity": giant_capacity(n, ns), "chunk_span": 0,
            "strata": np.zeros(nw, np.int64), "longest": np.zeros(nw, np.int64), "giants": np.zeros(nw, np.int64),
            "distinct": np.zeros(nw, np.int64)}
    if total == 0:
        return prof
    idx = onum.systematic_fixed(log_w, u0, ns)
    counts = np.zeros(nw * EM_WAVE_ITEMS, np.int64)
    counts[:n] = np.bincount(idx, minlength=n)
    counts = counts.reshape(nw, EM_WAVE_ITEMS)
    prof["strata"] = counts.sum(1)
    prof["longest"] = counts.max(1)
    prof["giants"] = (counts >= EM_GIANT).sum(1)
    prof["distinct"] = (counts > 0).sum(1)
    first = np.arange(0, ns, SYS_CHUNK)
    last = np.minimum(first + SYS_CHUNK, ns) - 1
    prof["chunk_span"] = int((idx[last] // SCAN_TILE - idx[first] // SCAN_TILE + 1).max())
    return prof
