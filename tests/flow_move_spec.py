"""Specification of the flow-proposal independence move of the AIS call as a small CPU program - TEST INFRASTRUCTURE, never
imported by the product.  The reference has no such move: like the SMC mode's, this definition is the project's own, and the
device follows it bit for bit (include/fabhip.h: fabhip_flow_move, fabhip_flow_moves_args).  numpy and float32 only.

One move at step j, with (c_q, c_p) the float32 anneal coefficients of beta_j (fabhip_anneal_coefs; `anneal_coefs` below
restates them) and (x', lq', lp', gq', gp') the Point of a fresh sample of the flow:

    r(lq, lp) = (c_q * lq + c_p * lp) - lq         float32, a * b + c un-fused, the expression order of fabhip_anneal_log_prob
    delta_i   = r(lq'_i, lp'_i) - r(lq_i, lp_i)
    accept_i  = i < n_valid  and  isfinite(lq'_i) and isfinite(lp'_i)  and  delta_i == delta_i  and  h_i > -delta_i

r is log [pi_beta / q]: the move is the Metropolis-Hastings test of an independence sampler with proposal q and target pi_beta,
so it leaves pi_beta invariant and the AIS weights are not touched.  h_i is a standard exponential draw (h = -log u: u < exp(delta)
is h > -delta), so neither exp nor log appears and spec and kernel agree bit for bit.

- An accepted row copies all five fields of the proposal (three for a gradient-free operator: x, log q, log p).
- Every other row is left bit-identical - the rows at and beyond n_valid among them.
- The move reports n_accept (an integer) and float32(n_accept) / float32(n_valid); with n_valid == 0 it reports 0.
- A current row with r = -inf (or NaN-free -inf densities) accepts any proposal with finite densities and finite r: delta = +inf.
  Where both r are -inf, delta is NaN and the row rejects.
- At beta = 0 with the AIS target p (c_q = 1, c_p = 0) and finite densities, r = (lq + 0 * lp) - lq is exactly 0 on both sides:
  delta = 0, h > -0 holds for every h > 0 and EVERY live row is accepted.  With alpha (p_target false) the same holds: beta = 0
  gives c_q = 1, c_p = 0 there too.  The tests use this.

`run_moves` applies k moves in sequence from given proposals and draws.
"""
from typing import NamedTuple, Optional, Sequence

import numpy as np

f32 = np.float32


def anneal_coefs(beta: float, alpha: float, p_target: bool):
    """(c_q, c_p) of fabhip_anneal_coefs: float64 arithmetic, rounded to float32 once."""
    beta, alpha = float(beta), float(alpha)
    if p_target:
        return f32(1.0 - beta), f32(beta)
    return f32((1.0 - beta) + beta * (1.0 - alpha)), f32(beta * alpha)


def ratio(c_q, c_p, lq, lp) -> np.ndarray:
    """r = (c_q lq + c_p lp) - lq with every operation rounded to float32 on its own."""
    lq, lp = np.asarray(lq, dtype=f32), np.asarray(lp, dtype=f32)
    with np.errstate(all="ignore"):
        a = (f32(c_q) * lq).astype(f32)
        b = (f32(c_p) * lp).astype(f32)
        return ((a + b).astype(f32) - lq).astype(f32)


class Point(NamedTuple):
    x: np.ndarray                       # [B, D] float32
    log_q: np.ndarray                   # [B]
    log_p: np.ndarray                   # [B]
    grad_log_q: Optional[np.ndarray]    # [B, D] or None (gradient-free operator)
    grad_log_p: Optional[np.ndarray]


class MoveResult(NamedTuple):
    point: Point
    accept: np.ndarray                  # [B] bool
    n_accept: int
    p_accept: np.float32


def _as_point(p) -> Point:
    g = lambda a: None if a is None else np.array(a, dtype=f32, copy=True)      # noqa: E731
    return Point(g(p[0]), g(p[1]), g(p[2]), g(p[3]), g(p[4]))


def accept_mask(c_q, c_p, cur_lq, cur_lp, prop_lq, prop_lp, h, n_valid: int) -> np.ndarray:
    cur_lq, prop_lq = np.asarray(cur_lq, dtype=f32), np.asarray(prop_lq, dtype=f32)
    prop_lp, h = np.asarray(prop_lp, dtype=f32), np.asarray(h, dtype=f32)
    B = cur_lq.shape[0]
    n_valid = min(max(int(n_valid), 0), B)
    with np.errstate(all="ignore"):
        delta = (ratio(c_q, c_p, prop_lq, prop_lp) - ratio(c_q, c_p, cur_lq, cur_lp)).astype(f32)
        ok = np.isfinite(prop_lq) & np.isfinite(prop_lp) & (delta == delta) & (h > -delta)
    return ok & (np.arange(B) < n_valid)


def move(cur, prop, h, c_q, c_p, n_valid: Optional[int] = None) -> MoveResult:
    """One move: `cur` / `prop` are (x, log_q, log_p, grad_log_q, grad_log_p) with both gradients None for a gradient-free
    operator; h [B] standard exponentials; n_valid None: all B rows."""
    cur, prop = _as_point(cur), _as_point(prop)
    B = cur.log_q.shape[0]
    n_valid = B if n_valid is None else min(max(int(n_valid), 0), B)
    acc = accept_mask(c_q, c_p, cur.log_q, cur.log_p, prop.log_q, prop.log_p, h, n_valid)
    new = []
    for a, b in zip(cur, prop):
        if a is None:
            new.append(None)
            continue
        a = a.copy()
        a[acc] = b[acc]
        new.append(a)
    n = int(acc.sum())
    frac = f32(n) / f32(n_valid) if n_valid > 0 else f32(0.0)
    return MoveResult(Point(*new), acc, n, f32(frac))


def run_moves(cur, proposals: Sequence, hs: Sequence, c_q, c_p, n_valid: Optional[int] = None):
    """k moves in sequence: proposals[m] is the Point of move m's proposal, hs[m] its draws.  Returns the final Point and the
    list of MoveResult."""
    results = []
    for prop, h in zip(proposals, hs):
        res = move(cur, prop, h, c_q, c_p, n_valid)
        results.append(res)
        cur = res.point
    return _as_point(cur), results
