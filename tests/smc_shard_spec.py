"""Specification of the SMC mode over SHARDED chains (parallel.ShardedAnnealedImportanceSampler(..., resample_across_ranks=True);
include/fabhip.h: fabhip_smc_shard_pack / fabhip_smc_shard_resample) as a small CPU program - TEST INFRASTRUCTURE, never imported
by the product.

There are R ranks.  Rank r holds b rows, of which the first n_r are live after the "chain init" filter.  The global live order is
the concatenation of the ranks' live rows in rank order: n0 = sum n_r, off_r = sum_{s<r} n_s.  Before transition j = 1 .. M, with
ONE uniform u_j shared by all ranks:

1. d = smc_spec.decide(concat(log_w_r[:n_r]), tau, u_j) - the single-device definition, unchanged.
2. d.resampled: rank r's live row i becomes the global live row d.ancestors[off_r + i] (x, log q, log p and, for HMC, both
   gradients); its log-weight becomes d.log_w_common.  Every rank keeps its count n_r; rows at and beyond n_r are untouched.
3. Otherwise the step is the identity.

By construction this is smc_spec.resample_step on the concatenated set, split back by the original counts.

The wire format of the state gather (`pack_state` / `unpack_state`) restates the device's: [b + 1, 3 D + 4] float32, row i < b =
x | grad log q | grad log p | log q, log p, log w, 0 and row b = n_r as an int32 bit pattern in its first word.
"""
from typing import List, Sequence

import numpy as np
import torch

import smc_spec
from oracle import ais as oais


def offsets(counts: Sequence[int]) -> List[int]:
    off = [0]
    for n in counts:
        off.append(off[-1] + int(n))
    return off


def _cat_live(points, log_ws, counts):
    cat = lambda name: (None if getattr(points[0], name) is None                                  # noqa: E731
                        else torch.cat([getattr(p, name)[:n] for p, n in zip(points, counts)]))
    pt = oais.Point(cat("x"), cat("log_q"), cat("log_p"), cat("grad_log_q"), cat("grad_log_p"))
    return pt, torch.cat([lw[:n] for lw, n in zip(log_ws, counts)])


def resample_step(points: Sequence[oais.Point], log_ws: Sequence[torch.Tensor], counts: Sequence[int], tau: float, u: float):
    """(points [R], log_ws [R], Decision) after the resampling step in front of a transition.  The inputs are not modified."""
    counts = [int(n) for n in counts]
    off = offsets(counts)
    glob_pt, glob_lw = _cat_live(points, log_ws, counts)
    d = smc_spec.decide(glob_lw.detach().numpy(), tau, u)
    out_p, out_w = [p.clone() for p in points], [lw.clone() for lw in log_ws]
    if not d.resampled:
        return out_p, out_w, d
    for r, n in enumerate(counts):
        idx = torch.as_tensor(np.asarray(d.ancestors[off[r]:off[r] + n]), dtype=torch.long)
        for name in ("x", "log_q", "log_p", "grad_log_q", "grad_log_p"):
            src = getattr(glob_pt, name)
            if src is not None:
                getattr(out_p[r], name)[:n] = src[idx]
        out_w[r][:n] = d.log_w_common
    return out_p, out_w, d


def pack_state(point: oais.Point, log_w: torch.Tensor, n_live: int) -> torch.Tensor:
    b, D = point.x.shape
    buf = torch.zeros((b + 1, 3 * D + 4), dtype=torch.float32)
    buf[:b, :D] = point.x
    if point.grad_log_q is not None:
        buf[:b, D:2 * D] = point.grad_log_q
        buf[:b, 2 * D:3 * D] = point.grad_log_p
    buf[:b, 3 * D], buf[:b, 3 * D + 1], buf[:b, 3 * D + 2] = point.log_q, point.log_p, log_w
    buf[b].view(torch.int32)[0] = int(n_live)
    return buf


def unpack_state(gathered: torch.Tensor, R: int, with_grad: bool):
    """gathered [R (b + 1), 3 D + 4] (or [R, b + 1, 3 D + 4]) -> (points [R], log_ws [R], counts [R])."""
    RW = gathered.shape[-1]
    g = gathered.reshape(R, -1, RW)
    b, D = g.shape[1] - 1, (RW - 4) // 3
    points, log_ws, counts = [], [], []
    for r in range(R):
        rows = g[r, :b]
        gq = rows[:, D:2 * D].clone() if with_grad else None
        gp = rows[:, 2 * D:3 * D].clone() if with_grad else None
        points.append(oais.Point(rows[:, :D].clone(), rows[:, 3 * D].clone(), rows[:, 3 * D + 1].clone(), gq, gp))
        log_ws.append(rows[:, 3 * D + 2].clone())
        counts.append(int(g[r, b].contiguous().view(torch.int32)[0]))
    return points, log_ws, counts


def resample_gathered(gathered: torch.Tensor, R: int, rank: int, with_grad: bool, tau: float, u: float):
    """What rank `rank` holds after the step, from the gathered send buffers: (point, log_w, Decision, counts)."""
    points, log_ws, counts = unpack_state(gathered, R, with_grad)
    out_p, out_w, d = resample_step(points, log_ws, counts, tau, u)
    return out_p[rank], out_w[rank], d, counts
