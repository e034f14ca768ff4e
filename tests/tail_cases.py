"""Named inputs of the tail of a chain phase - the ESS / log Z reduction (csrc/reduce_kernels.hip: msum_push, msum_push_chunk,
msum_merge, ess_partial_body, ess_final_body; k_ess_partial / k_ess_final and the same bodies inside k_tail_small) and the
compaction of the rows whose log_q or log_p is not finite (k_tail_small; csrc/ais_moves.hip: k_valid_scan, k_compact_scatter,
k_compact_copyback) - shared by test_tail_cases.py (CPU: every case reaches the branch it is listed for, judged from the two
restatements below and float64 torch alone) and test_gpu_tail.py (GPU: the kernels against float64 and `field[mask]`).
No test functions here.

The two restatements are written from the kernels' comments and code, vectorised over the threads of the grid.  The constants
restate the kernel constants that decide which path an element takes; a change on either side shows in the CPU file as a
branch that is no longer reached."""
import functools
import math
from collections import Counter, namedtuple

import numpy as np
import torch

from oracle import flow as oflow, numerical as onum

# ---- kernel constants (csrc/reduce_kernels.hip) ----
ESS_THREADS = 256           # constexpr int ESS_THREADS: threads per block of the partial pass
ESS_MAX_BLOCKS = 1024       # constexpr int ESS_MAX_BLOCKS: the grid's cap
ESS_PER_BLOCK = 1024        # grid_for(n, ESS_THREADS * 4, ESS_MAX_BLOCKS)
CHUNK = 16                  # msum_push_chunk<16>: values per thread per step of the float4 path
SCAN_TRIP = 1024            # rows per trip of the validity scan (TAIL_THREADS; k_valid_scan's 1024 threads)
TAIL_CHUNK = 32             # constexpr int TAIL_CHUNK: rows staged in LDS per step of the in-place move
TAIL_MAX_ROWS = 2048        # TAIL_MAX_BLOCKS * ESS_THREADS * 4: above it the separate kernels run
TAIL_LDS_BYTES = 48 * 1024  # (3 D + 4) * TAIL_CHUNK * 4 must fit: D <= 126, beyond FABHIP_MAX_DIM = 64 - no flow reaches it
CHUNK_FIRST_N = 1 << 22     # first n with n >= 16 * stride, stride = 256 * min(ceil(n / 1024), 1024)

# the tolerances of test_ess_logz_vs_golden (tests/test_gpu_parity.py)
ESS_RTOL = 1e-5
LOGZ_RTOL, LOGZ_ATOL = 1e-5, 1e-5

NINF, PINF, NAN = -np.inf, np.inf, np.nan


def ess_grid(n_cap: int) -> int:
    """grid_for(n_cap, 1024, 1024): blocks of the partial pass - from the CAPACITY, whatever *n_ptr says."""
    return min(max((n_cap + ESS_PER_BLOCK - 1) // ESS_PER_BLOCK, 1), ESS_MAX_BLOCKS)


def chunk_span(n_cap: int) -> int:
    """16 * stride: the elements one trip of the float4 path covers."""
    return CHUNK * ess_grid(n_cap) * ESS_THREADS


def chunk_elements(n_cap: int, thread: int, trip: int) -> np.ndarray:
    """The 16 element indices that thread `thread` of the grid reads in trip `trip` of the float4 path: four float4 loads
    `stride` float4s apart."""
    stride = ess_grid(n_cap) * ESS_THREADS
    h, k = np.divmod(np.arange(CHUNK), 4)
    return trip * CHUNK * stride + 4 * (h * stride + thread) + k


# ================================================================================================
# Restatement 1: the reduction
# ================================================================================================
def _exp32(d):
    """expf((float)d) as a double: the kernels form the argument in float64 (or float32 in the chunk), round it to float32
    and take a float32 exponential"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(np.asarray(d).astype(np.float32)).astype(np.float64)


def _sel(c, a, b):
    return np.where(c, a, b)


def _msum_push(st, x, act, cnt, mut):
    """msum_push on every thread with `act` set: x float64 [T]"""
    m, s1, s2 = st
    with np.errstate(invalid="ignore", over="ignore"):
        nan = act & (np.isnan(x) | np.isnan(m))
        pinf = act & ~nan & (x == PINF)
        ninf = act & ~nan & ~pinf & (x == NINF)
        rest = act & ~nan & ~pinf & ~ninf
        le = rest & (x <= m)
        gt = rest & ~le
        e = _exp32(x - m)
        r = _exp32(m - x)
        r2 = r if mut == "push_s2_r" else r * r
        cnt["scalar"] += int(act.sum())
        cnt["push_nan"] += int(nan.sum()); cnt["push_pinf"] += int(pinf.sum()); cnt["push_ninf"] += int(ninf.sum())
        cnt["push_le"] += int(le.sum()); cnt["push_gt"] += int(gt.sum())
        cnt["push_gt_late"] += int((gt & (m != NINF)).sum())
        if mut == "ninf_not_counted":
            cnt["_ninf_dropped"] += int(ninf.sum())
        nm = _sel(nan, NAN, _sel(pinf, PINF, _sel(gt, x, m)))
        ns1 = _sel(nan | pinf, NAN, _sel(le, s1 + e, _sel(gt, s1 * r + 1.0, s1)))
        ns2 = _sel(nan | pinf, NAN, _sel(le, s2 + e * e, _sel(gt, s2 * r2 + 1.0, s2)))
    return nm, ns1, ns2


def _msum_push_chunk(st, x, cnt, mut, trip):
    """msum_push_chunk<16> on every thread: x float32 [T, 16]"""
    m, s1, s2 = st
    with np.errstate(invalid="ignore", over="ignore"):
        xnan = np.isnan(x).any(axis=1)
        xpinf = (x == np.float32(PINF)).any(axis=1)
        cm = np.where(xnan, np.float32(NAN), np.max(np.where(np.isnan(x), np.float32(NINF), x), axis=1)).astype(np.float32)
        nan = xnan | np.isnan(m)
        pinf = ~nan & xpinf
        empty = ~nan & ~pinf & (cm == np.float32(NINF))
        rest = ~nan & ~pinf & ~empty
        ex = np.exp((x - cm[:, None]).astype(np.float32)).astype(np.float32)
        c1 = np.zeros(x.shape[0], np.float32)
        c2 = np.zeros(x.shape[0], np.float32)
        for i in range(CHUNK):                                   # the chunk's sums are float32, in index order
            c1 = (c1 + ex[:, i]).astype(np.float32)
            c2 = (c2 + (ex[:, i] * ex[:, i]).astype(np.float32)).astype(np.float32)
        md = cm.astype(np.float64)
        le = rest & (md <= m)
        gt = rest & ~le
        if mut == "chunk_keep_m":                                # the running maximum kept although the chunk's is larger
            le, gt = rest, rest & False
        r_le = _exp32(md - m)
        r_gt = _exp32(m - md)
        q_le = r_le if mut == "chunk_s2_r" else r_le * r_le
        q_gt = r_gt if mut == "chunk_s2_r" else r_gt * r_gt
        cnt["chunk"] += int(x.shape[0])
        cnt["chunk_nan"] += int((xnan & ~np.isnan(m)).sum()); cnt["chunk_pinf"] += int(pinf.sum())
        cnt["chunk_empty"] += int(empty.sum())
        cnt["chunk_le"] += int(le.sum()); cnt["chunk_gt"] += int(gt.sum())
        cnt["chunk_gt_late"] += int((gt & (m != NINF)).sum())        # a rescale of sums that hold something
        if trip > 0:
            cnt["chunk_gt_from_ninf_late"] += int((gt & (m == NINF)).sum())   # `a.m == -inf -> 0` behind an empty first chunk
        if mut == "ninf_not_counted":
            cnt["_ninf_dropped"] += int((x == np.float32(NINF)).sum())
        d1, d2 = c1.astype(np.float64), c2.astype(np.float64)
        nm = _sel(nan, NAN, _sel(pinf, PINF, _sel(gt, md, m)))
        ns1 = _sel(nan | pinf, NAN, _sel(le, s1 + r_le * d1, _sel(gt, s1 * r_gt + d1, s1)))
        ns2 = _sel(nan | pinf, NAN, _sel(le, s2 + q_le * d2, _sel(gt, s2 * q_gt + d2, s2)))
    return nm, ns1, ns2


def _msum_merge(a, b, cnt, mut):
    """msum_merge, element-wise over two arrays of partial states"""
    with np.errstate(invalid="ignore", over="ignore"):
        nan = np.isnan(a[0]) | np.isnan(b[0])
        m = np.fmax(a[0], b[0])
        ninf = ~nan & (m == NINF)
        pinf = ~nan & (m == PINF)
        ea, eb = np.exp(a[0] - m), np.exp(b[0] - m)
        if mut == "merge_no_rescale":
            ea, eb = np.ones_like(ea), np.ones_like(eb)
        s1 = a[1] * ea + b[1] * eb
        s2 = a[2] * ea * ea + b[2] * eb * eb
        if cnt is not None:
            cnt["merge_nan"] += int(nan.sum()); cnt["merge_ninf"] += int(ninf.sum()); cnt["merge_pinf"] += int(pinf.sum())
            cnt["merge"] += int((~nan & ~ninf & ~pinf).sum())
        return (_sel(nan, NAN, m), _sel(nan | pinf, NAN, _sel(ninf, 0.0, s1)), _sel(nan | pinf, NAN, _sel(ninf, 0.0, s2)))


def _tree(st, cnt, mut):
    """msum_block_reduce over the last axis (256 threads): sh[tid] = merge(sh[tid], sh[tid + s]), s = 128 .. 1"""
    s = st[0].shape[-1] >> 1
    while s > 0:
        st = _msum_merge(tuple(v[..., :s] for v in st), tuple(v[..., s:2 * s] for v in st), cnt, mut)
        s >>= 1
    return tuple(v[..., 0] for v in st)


Reduced = namedtuple("Reduced", "ess log_z n counts")


def reduce_restated(buf, n_cap: int, n=None, n_norm=None, offset: int = 0, mut=None) -> Reduced:
    """fabhip_ess_logz(buf[offset : offset + n_cap], n_cap, &n, n_norm) as the kernels compute it: the per-thread order of
    ess_partial_body for this (capacity, alignment), the block tree, ess_final_body.  `offset` is the position of the first
    value in a 16-byte aligned buffer (0: aligned, the float4 path may run; 1: the `[1:]` view, scalar loop only).
    Float64 running sums of exponentials formed from float32 arguments.  `counts`: pushes per branch.  `mut`: a one-line
    mutant (test_tail_cases.py lists them)."""
    lw = np.asarray(buf, np.float32)[offset:offset + n_cap]
    n = n_cap if n is None else int(n)
    n_read = n_cap if mut == "read_bait" else n
    n_norm = float(n) if n_norm is None else float(n_norm)
    cnt = Counter()
    nb = ess_grid(n_cap)
    stride = nb * ESS_THREADS
    tid = np.arange(stride)
    st = (np.full(stride, NINF), np.zeros(stride), np.zeros(stride))
    done, trip = 0, 0
    if (4 * offset) % 16 == 0:
        n16 = n_read // (CHUNK * stride) * (CHUNK * stride)
        for base in range(0, n16, CHUNK * stride):
            q = lw[base:base + CHUNK * stride].reshape(4, stride, 4)            # [h][tid][k] -> x[4 h + k]
            st = _msum_push_chunk(st, np.ascontiguousarray(q.transpose(1, 0, 2)).reshape(stride, CHUNK), cnt, mut, trip)
            trip += 1
        done = n16
    for i0 in range(done, n_read, stride):
        x = np.full(stride, NINF)
        k = min(stride, n_read - i0)
        x[:k] = lw[i0:i0 + k].astype(np.float64)
        st = _msum_push(st, x, tid < k, cnt, mut)
        trip += 1
    part = _tree(tuple(v.reshape(nb, ESS_THREADS) for v in st), cnt, mut)        # part[blockIdx.x]
    # ess_final_body: thread t merges part[t], part[t + 256], ... into the identity, then the tree
    pad = (-nb) % ESS_THREADS
    part = tuple(np.concatenate([v, np.full(pad, f)]).reshape(-1, ESS_THREADS) for v, f in zip(part, (NINF, 0.0, 0.0)))
    v = (np.full(ESS_THREADS, NINF), np.zeros(ESS_THREADS), np.zeros(ESS_THREADS))
    for row in range(part[0].shape[0]):
        v = _msum_merge(v, tuple(p[row] for p in part), None, mut)
    m, s1, s2 = (float(t) for t in _tree(v, None, mut))
    n_div = n_cap if mut == "ess_over_cap" else n
    if mut == "ninf_not_counted":
        n_div = n - cnt["_ninf_dropped"]
    with np.errstate(invalid="ignore", divide="ignore"):
        ess = np.float64(s1) * s1 / s2 / np.float64(n_div)
        lz_sum = PINF if m == PINF else m + np.log(np.float64(s1))              # logsumexp of a +inf weight is +inf
        log_z = lz_sum - np.log(np.float64(n if mut == "log_n" else n_norm))
    cnt.pop("_ninf_dropped", None)
    return Reduced(float(np.float32(ess)), float(np.float32(log_z)), n, cnt)


def reference64(values, n_norm):
    """(ESS, log Z) of oracle/numerical.py on float64 copies of the float32 values"""
    t = torch.as_tensor(np.asarray(values, np.float32)).double()
    ess = onum.effective_sample_size(t)
    lz = torch.logsumexp(t, dim=0) - math.log(n_norm)
    return float(ess), float(lz)


def reference32(values, n_norm):
    """the reference's own arithmetic: torch.softmax / logsumexp in float32"""
    t = torch.as_tensor(np.asarray(values, np.float32))
    return float(onum.effective_sample_size(t)), float(torch.logsumexp(t, dim=0) - math.log(n_norm))


def tol_units(got, ref):
    """(ESS error, log Z error) in units of the tolerance; inf where the non-finite patterns differ, 0 where both are the same
    non-finite value"""
    out = []
    for g, r, rt, at in ((got[0], ref[0], ESS_RTOL, 0.0), (got[1], ref[1], LOGZ_RTOL, LOGZ_ATOL)):
        if not (math.isfinite(g) and math.isfinite(r)):
            same = (math.isnan(g) and math.isnan(r)) or g == r
            out.append(0.0 if same else math.inf)
        else:
            out.append(abs(g - r) / (at + rt * abs(r)))
    return tuple(out)


# ================================================================================================
# The weight vectors
# ================================================================================================
# name | family (the README's table is per family) | capacity | n (None: no n_ptr) | offset | n_norm (None: n; a number; "3n") |
# build() -> float32 [capacity] | chunk: the float4 path runs | what the case is for
WCase = namedtuple("WCase", "name family n_cap n offset n_norm build chunk why")

EDGE_N = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2048, 2049)
N20, N22 = 1 << 20, 1 << 22
N_RAGGED = N22 + 4099
N_TWO = (1 << 23) + 5
N_PTRS = (1, 1025, N22, N22 + 1)


@functools.lru_cache(maxsize=1)
def _randn3_base():
    return (np.random.default_rng(1000).standard_normal(N_TWO + 8, dtype=np.float32) * np.float32(3)).astype(np.float32)


def randn3(n):
    """randn * 3: the first n of one seeded vector (drawn once: the long cases share it)"""
    return _randn3_base()[:n].copy()


def _poke(n, idx, val):
    def build():
        v = randn3(n)
        v[np.asarray(idx)] = val
        return v
    return build


def _first_chunks(n, threads, trips=(0,)):
    """whole chunks of the float4 path: every element that the threads `threads` read in the trips `trips`"""
    return np.concatenate([chunk_elements(n, t, k) for t in threads for k in trips])


def _bait(n_cap, n):
    """finite bait (far above every value in front of it), one NaN and one +inf beyond n"""
    def build():
        v = randn3(n_cap)
        v[n:] = np.float32(50.0) + np.arange(n_cap - n, dtype=np.float32) % np.float32(7)
        if n_cap - n >= 3:
            v[n + 1] = NAN
            v[n_cap - 1] = PINF
        return v
    return build


def weight_cases():
    c = []

    def add(name, family, n_cap, build, why, n=None, offset=0, n_norm=None):
        aligned = offset == 0
        n_used = n_cap if n is None else n
        c.append(WCase(name, family, n_cap, n, offset, n_norm, build, aligned and n_used >= chunk_span(n_cap), why))

    # -- sizes: one random vector per edge size (1 .. 3 blocks, every thread at most one push per block-stride)
    for n in EDGE_N:
        add(f"randn_{n}", "sizes", n, functools.partial(randn3, n), "block / thread edges of the scalar loop")
    add("randn_2^20", "capped grid", N20, functools.partial(randn3, N20), "the grid reaches its cap: 1024 blocks, 4 pushes per thread")
    add("randn_2^20+1", "capped grid", N20 + 1, functools.partial(randn3, N20 + 1), "capped grid, one thread takes a fifth push")
    add("randn_2^22-1", "capped grid", N22 - 1, functools.partial(randn3, N22 - 1), "the last all-scalar size: 16 pushes per thread but one")
    for n, tag, why in ((N22, "2^22", "first chunk-path size, nothing left for the scalar loop"),
                        (N_RAGGED, "2^22+4099", "one chunk trip and a ragged scalar remainder"),
                        (N_TWO, "2^23+5", "two chunk trips (the second rescales the first) and 5 scalar pushes")):
        add(f"randn_{tag}", "chunk path", n, functools.partial(randn3, n), why)
        add(f"randn_{tag}_unaligned", "unaligned", n, functools.partial(randn3, n),
            "the same values one float off 16-byte alignment: scalar loop only", offset=1)
    # -- ordering (per thread the pushes go up in steps of `stride`: 3 blocks at n = 2049, 3 pushes for the first thread)
    n = 2049
    add("ascending", "ordering", n, lambda: np.linspace(-40, 0, 2049, dtype=np.float32), "x > a.m on every push")
    add("descending", "ordering", n, lambda: np.linspace(0, -40, 2049, dtype=np.float32), "x <= a.m on every push after the first")
    add("max_in_the_middle", "ordering", n, lambda: (-np.abs(np.linspace(-20, 20, 2049))).astype(np.float32), "maximum exactly in the middle")
    add("ascending_2^20", "ordering", N20, lambda: np.linspace(-6, 0, N20, dtype=np.float32),
        "capped grid, four pushes per thread 1.5 apart: every rescale of the scalar loop carries weight")
    add("ascending_2^23+5", "ordering", N_TWO, lambda: np.linspace(-30, 0, N_TWO, dtype=np.float32),
        "the second chunk's maximum is the larger one on every thread: the chunk's `md > a.m` rescale")
    add("descending_2^23+5", "ordering", N_TWO, lambda: np.linspace(0, -30, N_TWO, dtype=np.float32),
        "the second chunk's maximum is the smaller one on every thread: the chunk's `md <= a.m` rescale")
    # -- closed forms
    add("constant", "closed form", 1025, lambda: np.full(1025, -3.25, np.float32), "ESS is exactly 1")
    add("one_dominant", "closed form", 1025, _poke(1025, 700, np.float32(400.0)), "ESS is 1 / n")
    add("spread_1e4", "spread / offsets", n, lambda: (np.random.default_rng(5).random(2049) * -1e4).astype(np.float32), "a spread of 1e4")
    add("offset_+1e6", "spread / offsets", n, lambda: (randn3(2049) + np.float32(1e6)).astype(np.float32), "offset +1e6")
    add("offset_-2e4", "spread / offsets", n, lambda: (randn3(2049) - np.float32(2e4)).astype(np.float32), "offset -2e4")
    add("pair_+-3e38", "spread / offsets", 257, _poke(257, [0, 1], np.array([3e38, -3e38], np.float32)),
        "x - m overflows to -inf in float32")
    add("pair_+-3e38_n2", "spread / offsets", 2, lambda: np.array([-3e38, 3e38], np.float32), "the pair alone: ESS 1 / 2")
    # -- -inf entries: weight 0, but they count in n
    add("ninf_few", "-inf", n, _poke(n, [0, 5, 1024, 2048], np.float32(NINF)), "a few -inf")
    add("ninf_all_but_one", "-inf", n, lambda: np.where(np.arange(2049) == 1500, np.float32(1.5), np.float32(NINF)).astype(np.float32),
        "all but one -inf: ESS 1 / n")
    add("ninf_all", "-inf", n, lambda: np.full(2049, NINF, np.float32), "all -inf: ESS NaN, log Z -inf")
    add("ninf_16_blocks", "-inf", N_RAGGED, _poke(N_RAGGED, np.arange(16 * 1000, 16 * 1200), np.float32(NINF)),
        "whole aligned 16-blocks of -inf inside chunks that hold other values")
    add("ninf_whole_chunks", "-inf", N_RAGGED, _poke(N_RAGGED, _first_chunks(N_RAGGED, (0, 63, 64, 262143)), np.float32(NINF)),
        "four threads' chunks hold nothing but -inf: the empty-chunk return")
    add("ninf_first_span", "-inf", N_TWO, _poke(N_TWO, np.arange(chunk_span(N_TWO)), np.float32(NINF)),
        "the whole first 16 * stride span is -inf: every thread's first chunk is empty, the second rescales from a.m == -inf")
    # -- NaN / +inf: NaN ESS (torch's softmax); log Z NaN for a NaN, +inf for a +inf (torch.logsumexp)
    add("nan_one", "special", n, _poke(n, 777, np.float32(NAN)), "one NaN, scalar loop")
    add("pinf_one", "special", n, _poke(n, 777, np.float32(PINF)), "one +inf, scalar loop")
    add("n_1", "special", 1, lambda: np.array([-7.5], np.float32), "n = 1: ESS 1, log Z the value")
    add("nan_in_chunk", "special", N_RAGGED, _poke(N_RAGGED, 3_000_001, np.float32(NAN)), "NaN in the chunk region")
    add("pinf_in_chunk", "special", N_RAGGED, _poke(N_RAGGED, 3_000_001, np.float32(PINF)), "+inf in the chunk region")
    add("nan_in_remainder", "special", N_RAGGED, _poke(N_RAGGED, N22 + 4000, np.float32(NAN)), "NaN in the scalar remainder behind the chunks")
    add("pinf_in_remainder", "special", N_RAGGED, _poke(N_RAGGED, N22 + 4000, np.float32(PINF)), "+inf in the scalar remainder behind the chunks")
    # -- n_ptr: the count comes from the device, the grid from the capacity; finite bait, a NaN and a +inf beyond the count
    for k in N_PTRS:
        add(f"n_ptr_{k}", "n_ptr", N_RAGGED, _bait(N_RAGGED, k), "n_ptr below the capacity: nothing beyond it is read", n=k)
    # -- n_norm
    add("n_norm_1_1025", "n_norm", 1025, functools.partial(randn3, 1025), "n_norm = 1.0 (the init tail's)", n_norm=1.0)
    add("n_norm_3n_1025", "n_norm", 1025, functools.partial(randn3, 1025), "n_norm = 3 n (the sharded call's)", n_norm="3n")
    add("n_norm_1_2^22+4099", "n_norm", N_RAGGED, functools.partial(randn3, N_RAGGED), "n_norm = 1.0 on the chunk path", n_norm=1.0)
    add("n_norm_3n_n_ptr", "n_norm", N_RAGGED, _bait(N_RAGGED, N22 + 1), "n_norm = 3 n with n from n_ptr", n=N22 + 1, n_norm="3n")
    return c


def n_used(case: WCase) -> int:
    return case.n_cap if case.n is None else case.n


def n_norm_of(case: WCase) -> float:
    n = n_used(case)
    return float(n) if case.n_norm is None else (3.0 * n if case.n_norm == "3n" else float(case.n_norm))


def buffer_of(case: WCase) -> np.ndarray:
    """the 16-byte aligned buffer whose `[offset:]` view holds the case's values (the slot in front is a finite bait)"""
    v = case.build()
    assert v.dtype == np.float32 and v.shape == (case.n_cap,)
    return np.concatenate([np.full(case.offset, 60.0, np.float32), v])


# ================================================================================================
# Restatement 2: the compaction
# ================================================================================================
def ranks_restated(lq, lp, n_in: int, mut=None):
    """k_valid_scan / the scan of k_tail_small: dest[r] = rank of row r among the valid rows, -1 for a dead row; trips of 1024
    rows, 16 waves of 64 lanes: rank = `running` (valid rows of earlier trips) + the valid rows of the waves in front (woff) +
    the valid lanes in front inside the wave (the ballot's popcount).  Returns (dest [n_in], n_out)."""
    lq, lp = np.asarray(lq, np.float32), np.asarray(lp, np.float32)
    dest = np.full(n_in, -1, np.int64)
    running = 0
    for base in range(0, n_in, SCAN_TRIP):
        k = min(SCAN_TRIP, n_in - base)
        v = np.zeros(SCAN_TRIP, bool)
        a, b = lq[base:base + k], lp[base:base + k]
        if mut == "valid_lq_only":
            v[:k] = np.isfinite(a)
        elif mut == "valid_not_nan":
            v[:k] = ~np.isnan(a) & ~np.isnan(b)
        else:
            v[:k] = np.isfinite(a) & np.isfinite(b)
        w = v.reshape(SCAN_TRIP // 64, 64).astype(np.int64)
        pre = np.cumsum(w, axis=1) - w                               # popcount(ballot & lanes in front)
        wsum = w.sum(axis=1)
        woff = np.cumsum(wsum) - (0 if mut == "woff_le" else wsum)   # sum over i < w  (mutant: i <= w)
        d = (0 if mut == "no_carry" else running) + woff[:, None] + pre
        dest[base:base + k] = np.where(v, d.reshape(-1), -1)[:k]
        running += int(wsum.sum())
    return dest, running


FIELDS = ("x", "lq", "lp", "gq", "gp", "log_w", "extra")


def compact_restated(fields: dict, n_in: int, form: str = "in_place", mut=None):
    """The move of the rows with finite log_q and log_p to the front, in order.  `fields`: x [B, D], lq, lp, log_w [B], gq / gp
    [B, D] or None (a Metropolis point), extra [B] or None.  form "in_place": k_tail_small - chunks of 32 rows through a staging
    buffer, a row is written only where its destination differs from its place; "staged": k_compact_scatter into a [B][3 D + 4]
    buffer and k_compact_copyback of its first n_out rows.  Nothing moves when no row is dead.  Rows in [n_out, B) are not
    written by either form.  Returns (the arrays after the move, n_out, dest)."""
    out = {k: (None if fields.get(k) is None else np.array(fields[k], np.float32, copy=True)) for k in FIELDS}
    dest, n_out = ranks_restated(out["lq"], out["lp"], n_in, mut)
    carried = [k for k in FIELDS if out[k] is not None]
    if mut == "no_extra":
        carried = [k for k in carried if k != "extra"]
    if mut == "no_grad":
        carried = [k for k in carried if k not in ("gq", "gp")]
    if n_out == n_in:
        return out, n_out, dest
    if form == "in_place":
        for r0 in range(0, n_in, TAIL_CHUNK):
            r = np.arange(r0, min(r0 + TAIL_CHUNK, n_in))
            stage = {k: out[k][r].copy() for k in carried}           # the chunk is read whole, then written
            d = dest[r]
            go = (d >= 0) & (d != r)
            for k in carried:
                out[k][d[go]] = stage[k][go]
    else:
        live = dest >= 0
        for k in carried:
            tmp = np.zeros_like(out[k])
            tmp[dest[live]] = out[k][:n_in][live]
            out[k][:n_out] = tmp[:n_out]
    return out, n_out, dest


# ================================================================================================
# Dead-row patterns, kinds of death, shapes
# ================================================================================================
def _span(n, lo, hi):
    m = np.zeros(n, bool)
    m[lo:min(hi, n)] = True
    return m


def _random_dead(n, k, seed):
    m = np.zeros(n, bool)
    m[np.random.default_rng(seed).choice(n, size=min(k, n), replace=False)] = True
    return m


# name -> (dead mask of n_in rows, stated number of survivors)
PATTERNS = {
    "none": (lambda n: np.zeros(n, bool), lambda n: n),
    "row_0": (lambda n: _span(n, 0, 1), lambda n: n - 1),
    "last_row": (lambda n: _span(n, n - 1, n), lambda n: n - 1),
    "all_but_first": (lambda n: ~_span(n, 0, 1), lambda n: 1),
    "all_but_last": (lambda n: ~_span(n, n - 1, n), lambda n: 1),
    "all": (lambda n: np.ones(n, bool), lambda n: 0),
    "alternating": (lambda n: np.arange(n) % 2 == 1, lambda n: (n + 1) // 2),
    "run_32_on_a_chunk": (lambda n: _span(n, 32, 64), lambda n: n - max(0, min(64, n) - 32)),        # one whole staging chunk
    "run_33_across_chunks": (lambda n: _span(n, 48, 81), lambda n: n - max(0, min(81, n) - 48)),     # rows 48 .. 80: three chunks
    "first_1024": (lambda n: _span(n, 0, 1024), lambda n: n - min(1024, n)),     # the first scan trip carries `running` = 0
    "random_1pc": (lambda n: _random_dead(n, max(1, round(0.01 * n)), 11 + n), lambda n: n - min(n, max(1, round(0.01 * n)))),
    "random_50pc": (lambda n: _random_dead(n, n // 2, 13 + n), lambda n: n - n // 2),
}

# (log_q, log_p) of a dead row; None: the row's finite value stays
KINDS = (("lq_nan", NAN, None), ("lq_ninf", NINF, None), ("lq_pinf", PINF, None),
         ("lp_nan", None, NAN), ("lp_ninf", None, NINF), ("lp_pinf", None, PINF),
         ("both_nan", NAN, NAN), ("both_mixed", PINF, NINF), ("nan_and_inf", NINF, NAN))

B_LIST = (1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
B_ALL_PATTERNS = (33, 1025, 2048, 2049)
D_LIST = (2, 6, 32, 60, 7)          # 7: the odd one (a GMM target; ManyWell pairs its coordinates)
THREE_PATTERNS = ("alternating", "run_33_across_chunks", "random_50pc")
BAIT_ROWS = 5

Shape = namedtuple("Shape", "B D n_in pattern")


def shapes():
    """every pattern at B in {33, 1025, 2048, 2049}, D = 6, with n_in = B and n_in = B - 5; every (B, D) with three patterns,
    n_in alternating between B and B - 5 (B - 5 < 1: B).  The one-launch form's LDS limit (3 D + 4) * 32 * 4 <= 48 KiB is
    D <= 126: no flow (FABHIP_MAX_DIM = 64) reaches it, so no D above it is listed."""
    out = []
    for B in B_ALL_PATTERNS:
        for p in PATTERNS:
            out += [Shape(B, 6, B, p), Shape(B, 6, B - BAIT_ROWS, p)]
    for B in B_LIST:
        for D in D_LIST:
            for i, p in enumerate(THREE_PATTERNS):
                n_in = B - BAIT_ROWS if (i + B + D) % 2 and B > BAIT_ROWS else B
                s = Shape(B, D, n_in, p)
                if s not in out:
                    out.append(s)
    return out


def dead_mask(shape: Shape) -> np.ndarray:
    """dead rows of the whole array [B]: the pattern over the first n_in rows; the bait rows behind them are alive-looking"""
    m = np.zeros(shape.B, bool)
    m[:shape.n_in] = PATTERNS[shape.pattern][0](shape.n_in)
    return m


def survivors_stated(shape: Shape) -> int:
    return PATTERNS[shape.pattern][1](shape.n_in)


def point_fields(shape: Shape, with_grad: bool = True, extra: bool = False, seed: int = 0) -> dict:
    """A constructed point of B rows: every value distinct and a function of its row (so that a row that went to the wrong
    place, or a column that stayed behind, shows), log_q / log_p of the dead rows set by the kinds of death in turn, finite
    distinct bait in the rows at and beyond n_in.  Also "kinds": the kind index of every dead row."""
    B, D, n_in = shape.B, shape.D, shape.n_in
    rng = np.random.default_rng(100 + seed + 7 * B + D)
    row = np.arange(B, dtype=np.float32)
    f = {"x": (row[:, None] + np.arange(D, dtype=np.float32)[None, :] / 64 + 0.25).astype(np.float32),
         "lq": (-3.0 - row / 1024 - (row % 7) * 0.5).astype(np.float32),
         "lp": (-5.0 + rng.standard_normal(B) * 3).astype(np.float32),
         "log_w": (rng.standard_normal(B) * 3).astype(np.float32),
         "gq": None, "gp": None, "extra": None}
    if with_grad:
        f["gq"] = (-f["x"] - 1.5).astype(np.float32)
        f["gp"] = (f["x"] * 2 + 5).astype(np.float32)
    if extra:
        f["extra"] = (row * 3 + 1).astype(np.float32)
    dead = dead_mask(shape)
    idx = np.flatnonzero(dead)
    kinds = np.full(B, -1)
    kinds[idx] = (np.arange(idx.size) + B) % len(KINDS)
    for k, (_, q, p) in enumerate(KINDS):
        sel = kinds == k
        if q is not None:
            f["lq"][sel] = q
        if p is not None:
            f["lp"][sel] = p
    f["kinds"] = kinds
    return f


# ---- the "chain init" tail: its dead rows come from the base noise ----------------------------------------------------------------
INIT_FLOW_SEED = 31
INIT_POISONS = (float("nan"), float("inf"), -float("inf"), 3e10)     # the last: finite, log_q stays finite, ManyWell's x^4 overflows
INIT_B = (37, 1025, 2048, 2049)
INIT_PATTERNS = ("row_0", "last_row", "alternating", "run_33_across_chunks", "random_50pc")


def init_flow(D):
    """The flow of the "chain init" tests: the oracle RealNVP as the reference initialises it (last coupling layers zero: a
    linear map), so that a base-noise entry of 3e10 keeps log_q finite (-0.5 * 9e20) while the target's x^4 overflows."""
    torch.manual_seed(INIT_FLOW_SEED + D)
    return oflow.make_realnvp(D, 2, 240 // D if D == 6 else 10)


def init_noise(B, D, pattern, seed=0):
    """(clean eps0, poisoned eps0, dead mask): the poisoned rows hold one of INIT_POISONS, in turn, in one coordinate"""
    g = torch.Generator().manual_seed(500 + seed + B + D)
    clean = torch.randn(B, D, generator=g)
    dead = PATTERNS[pattern][0](B)
    bad = clean.clone()
    for i, r in enumerate(np.flatnonzero(dead)):
        bad[r, (r + i) % D] = INIT_POISONS[i % len(INIT_POISONS)]
    return clean, bad, dead
