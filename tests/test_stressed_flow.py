"""The stressed-flow generator (tests/stressed_flow.py) and the fp32 CPU oracle on the flows it makes: what the GPU tests of
test_gpu_stressed_flow.py take for granted.  No GPU.

The oracle in float32 against its float64 copy, on every case the GPU test uses: log q and samples inside `helpers.close`, the
gradient d log q / dx inside the row rule with the oracle alone - every row passes clause (i) or lies within 4x the float64
spread of clause (iii) - and at most B // 8 rows per case are rows for which clause (iii) exists at all: rows beyond (i) on
which a float32 ReLU decision of the oracle differs from the float64 one (a kink).  Rows beyond (i) with the float64 decisions
are smooth rounding growth; the GPU test meets them with clause (ii)."""

import numpy as np
import pytest
import torch

import stressed_flow as sf
from helpers import close, worst, RTOL
from oracle import flow as oflow


@pytest.fixture(autouse=True)
def one_thread():
    """The fp32 oracle's sums follow the thread count; the GPU tests run it on one thread (tests/conftest.py), so this file does."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("D,K,nodes,act_norm", [(6, 3, 5, False), (5, 2, 4, True), (32, 10, 10, False), (2, 2, 8, True)])
def test_every_parameter_is_overwritten(D, K, nodes, act_norm):
    torch.manual_seed(1)
    nf = oflow.make_realnvp(D, K, nodes, act_norm=act_norm)
    before = {k: v.clone() for k, v in nf.state_dict().items()}
    nf64 = sf.stress_flow(nf, 2, 100.0, 1.0)
    after = nf.state_dict()
    assert set(after) == set(before)
    for k, v in after.items():
        if k.endswith((".eye", ".P", ".sign_S", ".data_dep_init_done")):
            continue                 # eye: a constant; P / sign_S: discrete, a re-draw can repeat them (checked below); the flag
        assert not torch.equal(v, before[k]), f"{k} kept its constructor value"
        assert bool(torch.isfinite(v).all())
    for k, p in nf.named_parameters():                         # the float64 copy holds the same float32-representable numbers
        assert torch.equal(dict(nf64.named_parameters())[k].float(), p) and dict(nf64.named_parameters())[k].dtype == torch.float64
    for f in nf.flows:
        if isinstance(f, oflow.InvertibleAffine):
            assert not torch.equal(f.P, torch.eye(D))
            assert D < 5 or (bool((f.sign_S > 0).any()) and bool((f.sign_S < 0).any()))
            assert torch.equal(f.P.sum(0), torch.ones(D)) and torch.equal(f.P.sum(1), torch.ones(D))
        if isinstance(f, oflow.ActNorm):
            assert float(f.data_dep_init_done) == 1.0
    # seeded: the same call gives the same flow
    torch.manual_seed(1)
    nf2 = oflow.make_realnvp(D, K, nodes, act_norm=act_norm)
    sf.stress_flow(nf2, 2, 100.0, 1.0)
    assert all(torch.equal(a, b) for a, b in zip(nf.state_dict().values(), nf2.state_dict().values()))


@pytest.mark.parametrize("D,K,nodes,cond", [(6, 3, 5, 10.0), (32, 10, 10, 100.0), (64, 2, 8, 100.0), (2, 4, 40, 100.0),
                                            (5, 2, 4, 1e4 ** 2), (60, 2, 4, 1e4 ** 2), (32, 2, 1, 1e2 ** 2)])
def test_condition_number_of_every_assembled_map(D, K, nodes, cond):
    nf, nf64 = sf.make_stressed(D, K, nodes, 7, cond, 1.0)
    want = cond ** (1.0 / K)
    n = 0
    for f in nf.flows:
        if isinstance(f, oflow.InvertibleAffine):
            with torch.no_grad():
                c = float(torch.linalg.cond(f._assemble_W().double()))
                ci = float(torch.linalg.cond(f._assemble_W(inverse=True).double()))
            assert abs(c - want) <= 0.01 * want, (c, want)
            assert abs(ci - want) <= 0.01 * want, (ci, want)
            n += 1
    assert n == K


def test_s_max_zero_gives_the_product_of_the_affine_maps():
    nf, nf64 = sf.make_stressed(6, 2, 5, 3, 1e4, 0.0)
    x = sf.density_points(nf64, 16, 1)
    W = torch.eye(6, dtype=torch.float64)
    with torch.no_grad():
        for f in nf64.flows:
            if isinstance(f, oflow.InvertibleAffine):
                W = W @ f._assemble_W(inverse=True)
            else:
                assert float(f.flows[1].param_map.net[-1].weight.abs().max()) == 0.0
        z = x @ torch.linalg.inv(W)
        lq = nf64.q0.log_prob(z) - torch.linalg.slogdet(W)[1]
        assert torch.allclose(lq, nf64.log_prob(x), rtol=1e-9, atol=1e-9)


def _cases():
    out = []
    for shp in sf.FLOW_SHAPES:
        out += [("b",) + shp + lv + (False,) for lv in sf.LEVELS if shp + lv not in sf.DROPPED]
        out.append(("b",) + shp + (100.0, 1.0, True))
    for shp in sf.AFFINE_SHAPES:
        out += [("a",) + shp + (c ** shp[1], 0.0, False) for c in sf.AFFINE_CONDS]
    for shp in sf.SMALL_TILE_SHAPES:
        out += [("c",) + shp + lv + (False,) for lv in sf.small_tile_levels(shp)]
    for shp in sf.PARAM_GRAD_SHAPES:
        out += [("d",) + shp + lv + (False,) for lv in sf.LEVELS[1:] if shp + lv not in sf.DROPPED]
    for D, K, nodes, an in sf.SAMPLE_GRAD_SHAPES:
        out.append(("e", D, K, nodes, 100.0, 1.0, an))
    seen, uniq = set(), []
    for c in out:                                              # (one evaluation per distinct flow: the groups share shapes)
        if c[1:] not in seen:
            seen.add(c[1:]); uniq.append(c)
    return uniq


@pytest.mark.parametrize("group,D,K,nodes,cond,s_max,act_norm", _cases())
def test_fp32_oracle_stays_inside_the_row_rule(group, D, K, nodes, cond, s_max, act_norm):
    c = sf.oracle_case(D, K, nodes, cond, s_max, act_norm)
    for k in ("x", "lq64", "g64", "xs64", "ls64"):
        assert bool(torch.isfinite(c[k]).all()), f"float64 oracle: {k} is not finite"
    # the sampling direction at every case; the density direction wherever the GPU test checks it
    assert close(c["xs32"], c["xs64"], RTOL), f"sample x: {worst(c['xs32'], c['xs64']):.2f} tol units"
    assert close(c["ls32"], c["ls64"], RTOL), f"sample log q: {worst(c['ls32'], c['ls64']):.2f} tol units"
    if group == "a" and (cond ** (1.0 / K)) > sf.AFFINE_DENSITY_MAX_COND:
        return
    assert close(c["lq32"], c["lq64"], RTOL), f"log q: {worst(c['lq32'], c['lq64']):.2f} tol units"
    e, u = sf.row_errors(c["g32"], c["g64"])
    beyond = u > 1.0
    inside = np.ones_like(beyond)
    if beyond.any():
        rows = np.nonzero(beyond)[0]
        scale = max(1.0, float(c["g64"].abs().max()))
        inside[rows] = e[rows] <= 4 * sf.grad_spread(c["nf64"], c["x"][rows], c["g64"][rows], scale, seed=int(rows[0]))
    flipped = (sf.relu_decisions(c["nf"], c["x"].float()) != sf.relu_decisions(c["nf64"], c["x"])).any(1).numpy()
    msg = (f"gradient: worst {u.max():.1f} tol units, {int(beyond.sum())} rows beyond (i), {int((beyond & flipped).sum())} of them "
           f"at a kink, {int((beyond & ~inside).sum())} outside 4x the float64 spread")
    print(msg)
    assert not (beyond & ~inside).any(), msg
    assert int((beyond & flipped).sum()) <= sf.B // 8, msg
