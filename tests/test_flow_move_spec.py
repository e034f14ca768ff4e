"""The flow-proposal independence move's definition (tests/flow_move_spec.py) on the CPU: the rule's edge cases and the
invariance of pi_beta under repeated moves."""
import numpy as np

import flow_move_spec as spec

f32 = np.float32


def _point(B, D, seed, with_grad=True):
    rng = np.random.default_rng(seed)
    g = lambda *s: rng.standard_normal(s).astype(f32)      # noqa: E731
    return (g(B, D), g(B), g(B), g(B, D) if with_grad else None, g(B, D) if with_grad else None)


def _same(a, b):
    return a is b is None or (a is not None and b is not None and np.array_equal(a, b, equal_nan=True) and a.dtype == b.dtype)


def test_every_live_row_is_accepted_at_beta_zero():
    B, D = 37, 5
    for p_target, alpha in ((True, 0.0), (False, 2.0)):
        c_q, c_p = spec.anneal_coefs(0.0, alpha, p_target)
        assert (c_q, c_p) == (f32(1.0), f32(0.0))
        cur, prop = _point(B, D, 1), _point(B, D, 2)
        h = np.random.default_rng(3).exponential(size=B).astype(f32)
        h[0] = np.nextafter(f32(0), f32(1))                 # the smallest positive draw still accepts: delta is exactly 0
        res = spec.move(cur, prop, h, c_q, c_p)
        assert res.accept.all() and res.n_accept == B and res.p_accept == f32(1.0)
        for a, b in zip(res.point, prop):
            assert _same(a, b)


def test_non_finite_proposal_densities_are_rejected():
    B, D = 8, 3
    c_q, c_p = spec.anneal_coefs(0.3, 2.0, False)
    cur, prop = _point(B, D, 4), list(_point(B, D, 5))
    prop[1][0], prop[1][1], prop[1][2] = np.nan, -np.inf, np.inf          # log q'
    prop[2][3], prop[2][4] = np.nan, -np.inf                              # log p'
    h = np.full(B, 1e30, dtype=f32)                                       # (finite rows would accept whatever delta is)
    res = spec.move(cur, prop, h, c_q, c_p)
    assert not res.accept[:5].any() and res.accept[5:].all()
    assert res.n_accept == 3 and res.p_accept == f32(3) / f32(8)
    for a, b in zip(res.point, cur):
        assert _same(a[:5], b[:5])


def test_a_current_row_at_minus_infinity_accepts_a_finite_proposal():
    B, D = 4, 2
    c_q, c_p = spec.anneal_coefs(1.0, 0.0, True)
    cur, prop = list(_point(B, D, 6)), _point(B, D, 7)
    cur[2][:] = -np.inf                                                   # log p = -inf: r = -inf
    h = np.full(B, 1e30, dtype=f32)
    res = spec.move(cur, prop, h, c_q, c_p)
    assert res.accept.all()


def test_both_minus_infinity_rejects():
    # r' = -inf with FINITE densities: c_p * lp' overflows (alpha = 2, beta = 1: c_p = 2)
    c_q, c_p = spec.anneal_coefs(1.0, 2.0, False)
    B, D = 3, 2
    cur, prop = list(_point(B, D, 8)), list(_point(B, D, 9))
    cur[2][:] = -np.inf
    prop[2][:] = f32(-3e38)
    assert np.isfinite(prop[2]).all() and np.isneginf(spec.ratio(c_q, c_p, prop[1], prop[2])).all()
    res = spec.move(cur, prop, np.full(B, 1e30, dtype=f32), c_q, c_p)
    assert not res.accept.any() and res.n_accept == 0 and res.p_accept == f32(0)
    for a, b in zip(res.point, cur):
        assert _same(a, b)


def test_rows_at_and_beyond_n_valid_are_untouched():
    B, D = 10, 4
    c_q, c_p = spec.anneal_coefs(0.0, 0.0, True)
    for with_grad in (True, False):
        cur, prop = _point(B, D, 10, with_grad), _point(B, D, 11, with_grad)
        res = spec.move(cur, prop, np.ones(B, dtype=f32), c_q, c_p, n_valid=7)
        assert res.accept[:7].all() and not res.accept[7:].any()
        assert res.n_accept == 7 and res.p_accept == f32(1.0)
        for a, b, c in zip(res.point, cur, prop):
            assert _same(a if a is None else a[7:], b if b is None else b[7:])
            assert _same(a if a is None else a[:7], c if c is None else c[:7])


def test_n_valid_zero_reports_zero():
    B, D = 6, 2
    c_q, c_p = spec.anneal_coefs(0.0, 0.0, True)
    cur, prop = _point(B, D, 12), _point(B, D, 13)
    res = spec.move(cur, prop, np.ones(B, dtype=f32), c_q, c_p, n_valid=0)
    assert res.n_accept == 0 and res.p_accept == f32(0) and res.p_accept.dtype == f32 and not res.accept.any()
    for a, b in zip(res.point, cur):
        assert _same(a, b)


def test_run_moves_is_the_sequence_of_moves():
    B, D, k = 12, 3, 3
    c_q, c_p = spec.anneal_coefs(0.5, 0.0, True)
    cur = _point(B, D, 20)
    props = [_point(B, D, 21 + m) for m in range(k)]
    hs = [np.random.default_rng(30 + m).exponential(size=B).astype(f32) for m in range(k)]
    final, results = spec.run_moves(cur, props, hs, c_q, c_p, n_valid=10)
    step = cur
    for m in range(k):
        r = spec.move(step, props[m], hs[m], c_q, c_p, n_valid=10)
        assert np.array_equal(r.accept, results[m].accept) and r.n_accept == results[m].n_accept
        step = r.point
    for a, b in zip(final, step):
        assert _same(a, b)


def test_moves_leave_the_target_invariant_and_reach_it():
    """1-D, q = N(0, 1), p = N(1.5, 0.6^2), beta = 1, 4096 chains started from q, 40 moves: the final mean within 0.05 of 1.5
    and the final variance within 0.06 of 0.36 (a numpy simulation of exactly this rule over 20 seeds gave at most 0.016 and
    0.020; the standard error of the mean is 0.009; mean acceptance about 0.23)."""
    rng = np.random.default_rng(12345)
    B, k, mu, sig = 4096, 40, 1.5, 0.6

    def lq(x):
        return (-0.5 * x * x - 0.5 * np.log(2 * np.pi)).astype(f32)

    def lp(x):
        return (-0.5 * ((x - mu) / sig) ** 2 - np.log(sig) - 0.5 * np.log(2 * np.pi)).astype(f32)

    def point(x):
        x = x.astype(f32).reshape(B, 1)
        return (x, lq(x[:, 0].astype(np.float64)), lp(x[:, 0].astype(np.float64)), None, None)

    c_q, c_p = spec.anneal_coefs(1.0, 0.0, True)
    cur = point(rng.standard_normal(B))
    props = [point(rng.standard_normal(B)) for _ in range(k)]
    hs = [rng.exponential(size=B).astype(f32) for _ in range(k)]
    final, results = spec.run_moves(cur, props, hs, c_q, c_p)
    x = final.x[:, 0].astype(np.float64)
    acc = float(np.mean([r.p_accept for r in results]))
    print(f"mean {x.mean():.4f} var {x.var():.4f} mean acceptance {acc:.3f}")
    assert abs(x.mean() - mu) <= 0.05
    assert abs(x.var() - sig * sig) <= 0.06
