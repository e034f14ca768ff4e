"""The tail of a chain phase on the GPU, on the cases of tests/tail_cases.py (asserted on the CPU by test_tail_cases.py):

(a) the reduction kernels (k_ess_partial / k_ess_final through fabhip::ess_logz and fa.ess_and_log_z) against the float64
    statement of oracle/numerical.py at the tolerances of test_ess_logz_vs_golden - scalar loop and float4 path, capped grid,
    unaligned pointers, n_ptr with bait behind it, n_norm, -inf / NaN / +inf;
(b) the "chain end" tail (FABHIP_AIS_FINISH alone on a constructed point) on both routes - k_tail_small (FABHIP_OPT_FUSED_TAIL = 1,
    B <= 2048) and k_valid_scan / k_compact_* / k_ess_* - against `field[mask]`, bit for bit, HMC and Metropolis points;
(c) the "chain init" tail: rows that die from the base noise, against a run of the same shape on clean noise;
(d) one whole call against oracle/ais.py with half the chains dying at init.

Lines starting with "MEASURE" give errors in units of the tolerance, the float32 formula of the reference beside the kernels."""
import math

import numpy as np
import pytest
import torch

import tail_cases as tc
from helpers import close, worst, RTOL
from oracle import ais as oais, numerical as onum, targets as otgt
from test_gpu_parity import hip_flow_from_oracle, seeded_flow, DEV

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _ops      # noqa: E402

CASES = tc.weight_cases()
BY_NAME = {c.name: c for c in CASES}
SENTINEL = -12345.0


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def device_view(case, buf):
    """the case's values on the device: a view at `offset` floats into a fresh (16-byte aligned) allocation"""
    d = torch.from_numpy(buf).to(DEV)
    v = d[case.offset:]
    assert v.is_contiguous() and v.numel() == case.n_cap and v.data_ptr() % 16 == 4 * case.offset
    return v


def statement64(v, n, n_norm):
    """oracle/numerical.py in float64 on the first n values (plain torch on the device: no kernel of this package)"""
    t = v[:n].double()
    return float(onum.effective_sample_size(t)), float(torch.logsumexp(t, dim=0) - math.log(n_norm))


def statement32(v, n, n_norm):
    t = v[:n]
    return float(onum.effective_sample_size(t)), float(torch.logsumexp(t, dim=0) - math.log(n_norm))


def run_weight_case(name):
    """(out float32[3] on the host, float64 statement, float32 formula) of one weight case: every caller launches its own"""
    c = BY_NAME[name]
    ops = _ops.load()
    buf = tc.buffer_of(c)
    v = device_view(c, buf)
    n, n_norm = tc.n_used(c), tc.n_norm_of(c)
    n_ptr = None if c.n is None else torch.tensor([c.n], dtype=torch.int32, device=DEV)
    out = ops.ess_logz(v, n_ptr, n_norm)
    again = ops.ess_logz(v, n_ptr, n_norm)
    assert torch.equal(bits(out), bits(again)), f"{name}: two calls differ"
    if c.n is None:                                           # the Python entry point: the same kernels on the same pointer
        assert torch.equal(bits(fa.ess_and_log_z(v, n_norm)), bits(out))
    else:                                                     # the bait beyond n_ptr changes no bit: zeros behind the count
        z = buf.copy()
        z[c.offset + c.n:] = 0.0
        assert np.isnan(buf[c.offset + c.n:]).any()
        assert torch.equal(bits(ops.ess_logz(device_view(c, z), n_ptr, n_norm)), bits(out)), f"{name}: the bait was read"
    return out.cpu(), statement64(v, n, n_norm), statement32(v, n, n_norm)


# ---- (a) the reduction kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_ess_logz_kernels_against_float64(name):
    c = BY_NAME[name]
    out, ref64, ref32 = run_weight_case(name)
    got = (float(out[0]), float(out[1]))
    u, u32 = tc.tol_units(got, ref64), tc.tol_units(ref32, ref64)
    print(f"MEASURE a | {c.family} | {name} | HIP ess {u[0]:.2e} logz {u[1]:.2e} | fp32 formula ess {u32[0]:.2e} logz {u32[1]:.2e}")
    assert max(u) <= 1.0, (name, got, ref64, u)              # NaN / +-inf where float64 torch gives them: tol_units is inf else
    assert bits(out[2:3]).item() == bits(torch.tensor([float(tc.n_used(c))])).item()


@pytest.mark.parametrize("tag", ["2^22", "2^22+4099", "2^23+5"])
def test_aligned_and_unaligned_copies_agree(tag):
    """the float4 path (aligned) and the scalar loop (one float off) on the same values: both inside the tolerance of float64
    (asserted above, and here on this test's own launches) and of each other; their bits may differ (another order of float32 and float64 additions)"""
    (a, ref, _), (b, _, _) = run_weight_case(f"randn_{tag}"), run_weight_case(f"randn_{tag}_unaligned")
    assert max(tc.tol_units((float(a[0]), float(a[1])), ref)) <= 1.0 and max(tc.tol_units((float(b[0]), float(b[1])), ref)) <= 1.0
    u = tc.tol_units((float(a[0]), float(a[1])), (float(b[0]), float(b[1])))
    print(f"MEASURE a | aligned vs unaligned | {tag} | ess {u[0]:.2e} logz {u[1]:.2e} | bits differ: {not torch.equal(bits(a), bits(b))}")
    assert max(u) <= 1.0 and a[2] == b[2]


# ---- (b) the "chain end" tail on constructed points -------------------------------------------------------------------------------
_samplers = {}


def chain_end_sampler(D, hmc):
    """a sampler whose flow only carries D (the smallest one the kernels take) - FABHIP_AIS_FINISH runs no flow"""
    if (D, hmc) not in _samplers:
        torch.manual_seed(40 + D)
        flow = fa.RealNVP(D, 2, max(1, -(-16 // D))).to(DEV).requires_grad_(False)
        target = fa.GMM(D, 3, 1.0).to(DEV) if D % 2 else fa.ManyWellEnergy(D)
        if hmc:
            op = fa.HamiltonianMonteCarlo(1, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.1, n_outer=1,
                                          L=1).to(DEV)
        else:
            op = fa.Metropolis(1, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, n_updates=1).to(DEV)
        _samplers[(D, hmc)] = fa.AnnealedImportanceSampler(flow, target.log_prob, op, p_target=False, alpha=2.0,
                                                           n_intermediate_distributions=1)
    return _samplers[(D, hmc)]


def chain_end(ais, shape, f, hmc, route):
    """FABHIP_AIS_FINISH alone on the constructed point `f`: every array afterwards, on the host.  `stats` is the one buffer
    of this call the caller owns (the index and staging workspaces are the op's own scratch): pre-filled with a sentinel."""
    ops = _ops.load()
    ops.set_option(_ops.OPT_FUSED_TAIL, route)
    st = ais.new_phase_state(shape.B)
    names = ("x", "lq", "lp", "log_w") + (("gq", "gp") if hmc else ())
    for k in names:
        st[k].copy_(torch.from_numpy(f[k]))
    assert hmc or (st["gq"] is None and st["gp"] is None)
    st["stats"].fill_(SENTINEL)
    st["n_valid"].copy_(torch.tensor([shape.n_in, -77], dtype=torch.int32))
    ais.enqueue_phase(st, 2, 1, 0, logging=False)
    torch.cuda.synchronize()
    out = {k: st[k].cpu().numpy() for k in names}
    out["stats"], out["n_valid"] = st["stats"].cpu().numpy(), st["n_valid"].cpu().numpy()
    return out


def check_chain_end(shape, hmc):
    ais = chain_end_sampler(shape.D, hmc)
    f = tc.point_fields(shape, with_grad=hmc)
    valid = np.zeros(shape.B, bool)
    valid[:shape.n_in] = ~tc.dead_mask(shape)[:shape.n_in]
    n_out = int(valid.sum())
    assert n_out == tc.survivors_stated(shape)
    outs = {}
    try:
        for route in (1, 0):
            outs[route] = chain_end(ais, shape, f, hmc, route)
    finally:
        _ops.load().set_option(_ops.OPT_FUSED_TAIL, 1)
    i32 = lambda a: np.ascontiguousarray(a).view(np.int32)                                           # noqa: E731
    for route, o in outs.items():
        tag = (shape, "hmc" if hmc else "metropolis", f"route {route}")
        assert o["n_valid"].tolist() == [shape.n_in, n_out], tag
        for k in f:
            if k not in o:
                continue
            assert np.array_equal(i32(o[k][:n_out]), i32(f[k][valid])), (tag, k, "survivors")
            assert np.array_equal(i32(o[k][n_out:]), i32(f[k][n_out:])), (tag, k, "rows at and beyond n_out are not written")
        assert np.all(o["stats"][:3] == SENTINEL) and np.all(o["stats"][6:] == SENTINEL), tag
        ess, lz, cnt = (float(v) for v in o["stats"][3:6])
        assert cnt == n_out, tag
        if n_out == 0:                                        # all dead: include/fabhip.h (outside the reference's domain)
            assert math.isnan(ess) and lz == -math.inf, tag
        else:
            ref = tc.reference64(f["log_w"][valid], float(shape.B))
            u = tc.tol_units((ess, lz), ref)
            assert max(u) <= 1.0, (tag, (ess, lz), ref, u)
    # both routes: the same bits everywhere (above 2048 rows there is one route only: the option is not read)
    for k in outs[1]:
        assert np.array_equal(i32(outs[1][k]), i32(outs[0][k])), (shape, k, "routes differ")
    return outs[1]


B_D = sorted({(s.B, s.D) for s in tc.shapes()})


@pytest.mark.parametrize("B,D", B_D)
def test_chain_end_tail_is_field_of_mask_on_both_routes(B, D):
    """every listed (n_in, pattern) of this (B, D): an HMC point; at D = 6 and the odd D also a Metropolis point (no gradient
    fields: `gq == nullptr` in both compactions)"""
    for shape in tc.shapes():
        if (shape.B, shape.D) != (B, D):
            continue
        check_chain_end(shape, True)
        if D in (6, 7):
            check_chain_end(shape, False)


# ---- (c) the "chain init" tail ----------------------------------------------------------------------------------------------------
# "hmc<n>": HMC with FABHIP_OPT_TILE_SHAPE = n at every B (left alone the call takes 4-chain tiles up to 1152 chains, 8-chain above)
OPERATORS = ("hmc4", "hmc8", "hmc16", "metropolis")
_init = {}


def init_sampler(D, op):
    if (D, op) not in _init:
        flow = hip_flow_from_oracle(tc.init_flow(D))
        target = fa.ManyWellEnergy(D)
        if op == "metropolis":
            t = fa.Metropolis(1, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, n_updates=1, eval_mode=True).to(DEV)
        else:                                  # (eval_mode: the step sizes stay, so that every call of one sampler is the same call)
            t = fa.HamiltonianMonteCarlo(1, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.05, n_outer=1,
                                         L=1, eval_mode=True).to(DEV)
        _init[(D, op)] = fa.AnnealedImportanceSampler(flow, target.log_prob, t, p_target=False, alpha=2.0,
                                                      n_intermediate_distributions=1)
    return _init[(D, op)]


def chain_init(ais, B, D, hmc, eps0, route):
    """(the point after FABHIP_AIS_INIT alone, the init tail's outputs of a whole call with want_base) on the base noise eps0"""
    ops = _ops.load()
    ops.set_option(_ops.OPT_FUSED_TAIL, route)
    g = torch.Generator().manual_seed(7)
    na = torch.randn(1, 1, B, D, generator=g).to(DEV)
    nb = (torch.empty(1, 1, B).exponential_(1.0, generator=g) if hmc else torch.rand(1, 1, B, generator=g)).to(DEV)
    st = ais.new_phase_state(B, eps0.to(DEV), na, nb)
    st["stats"].fill_(SENTINEL)
    ais.enqueue_phase(st, 1, 1, 0, logging=False)
    torch.cuda.synchronize()
    names = ("x", "lq", "lp", "log_w") + (("gq", "gp") if hmc else ())
    point = {k: st[k].clone() for k in names}
    point["stats"], point["n_valid"] = st["stats"].clone(), st["n_valid"].clone()
    _, _, n_valid, stats, base_x, base_lw = ais.run(B, eps0.to(DEV), na, nb, want_base=True)
    torch.cuda.synchronize()
    return point, {"n_valid": n_valid.clone(), "stats": stats.clone(), "base_x": base_x.clone(), "base_lw": base_lw.clone()}


@pytest.mark.parametrize("op", OPERATORS)
@pytest.mark.parametrize("B,D", [(B, 6) for B in tc.INIT_B] + [(B, 32) for B in tc.INIT_B])
def test_chain_init_tail_keeps_the_survivors_of_a_clean_run(B, D, op):
    """Rows die from the base noise (NaN, +-inf, and 3e10: log_q finite, log_p overflows - test_tail_cases.py); the reference
    is a run of the same shape on clean noise: rows do not mix inside a tile, so the survivors are that run's rows [mask] bit
    for bit - the point, base_x, base_log_w (the compaction's `extra` column), and the statistics over log_p - log_q (`diff`)."""
    hmc = op != "metropolis"
    ais = init_sampler(D, op)
    ops = _ops.load()
    patterns = tc.INIT_PATTERNS
    try:
        ops.set_option(_ops.OPT_TILE_SHAPE, int(op[3:]) if hmc else 0)
        clean_eps = tc.init_noise(B, D, patterns[0])[0]
        cp, cr = chain_init(ais, B, D, hmc, clean_eps, 1)
        assert cp["n_valid"][0].item() == B and cr["n_valid"][0].item() == B
        diff_clean = cp["lp"] - cp["lq"]                       # float32, k_sub's subtraction
        for pattern in patterns:
            clean, bad, dead = tc.init_noise(B, D, pattern)
            assert torch.equal(clean, clean_eps)
            mask = torch.from_numpy(~dead).to(DEV)
            n0 = int(mask.sum())
            ref = statement64(diff_clean[mask], n0, 1.0)
            res = {}
            for route in (1, 0):
                p, r = chain_init(ais, B, D, hmc, bad, route)
                tag = (B, D, op, pattern, route)
                assert p["n_valid"][0].item() == n0 and r["n_valid"][0].item() == n0, tag
                for k in cp:
                    if k not in ("stats", "n_valid"):
                        assert torch.equal(bits(p[k][:n0]), bits(cp[k][mask])), (tag, k)
                assert torch.equal(bits(r["base_x"][:n0]), bits(cr["base_x"][mask])), tag
                assert torch.equal(bits(r["base_lw"][:n0]), bits(cr["base_lw"][mask])), tag
                for stats in (p["stats"], r["stats"]):
                    u = tc.tol_units((float(stats[0]), float(stats[1])), ref)
                    assert max(u) <= 1.0 and float(stats[2]) == n0, (tag, stats[:3].tolist(), ref, u)
                    assert torch.all(stats[6:16] == 0), tag
                assert torch.all(p["stats"][3:6] == SENTINEL), tag
                res[route] = (p, r)
            for a, b in zip(res[1], res[0]):                   # both routes: the same bits over the WHOLE arrays (launch.h) - the
                for k in a:                                    # point, base_x, the `extra` column base_log_w, stats, n_valid
                    assert torch.equal(bits(a[k]), bits(b[k])), (B, D, op, pattern, k, "routes differ")
    finally:
        ops.set_option(_ops.OPT_FUSED_TAIL, 1)
        ops.set_option(_ops.OPT_TILE_SHAPE, 0)


# ---- (d) one whole call against the oracle ---------------------------------------------------------------------------------------
def test_whole_call_with_half_the_chains_dying_at_init_against_the_oracle():
    """M = 2, D = 6, B = 40 as test_nan_rows_are_compacted_like_the_reference, with 20 chains dying at init (row 0 and row B - 1
    among them): x, log_w and the logged statistics against oracle/ais.py on the same noise, both routes bit-equal."""
    D, M, B = 6, 2, 40
    nf = seeded_flow(D, 2, 5, 77)
    hf = hip_flow_from_oracle(nf)
    target = fa.ManyWellEnergy(D)
    torch.manual_seed(1)
    eps0 = torch.randn(B, D)
    dead = [r for r in range(0, B - 2, 2)] + [B - 1]
    assert len(dead) == B // 2 and 0 in dead and B - 1 in dead
    for i, r in enumerate(dead):
        eps0[r, i % D] = (float("nan"), float("inf"), -float("inf"))[i % 3]
    noise_p = torch.randn(M, 1, B, D)
    noise_e = torch.empty(M, 1, B).exponential_()
    ohmc = oais.HMC(M, D, nf.log_prob, otgt.ManyWell(D).log_prob, alpha=2.0, p_target=False, epsilon=0.1, eval_mode=True)
    oa = oais.AIS(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, otgt.ManyWell(D).log_prob, ohmc, False, 2.0, M)
    opt, olw, oinfo = oa.sample_and_log_weights(eps0, noise_p, noise_e)
    assert opt.x.shape[0] == B - len(dead)
    ops = _ops.load()
    res = {}
    try:
        for route in (1, 0):
            ops.set_option(_ops.OPT_FUSED_TAIL, route)
            hmc = fa.HamiltonianMonteCarlo(M, D, hf.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.1,
                                           eval_mode=True).to(DEV)
            ais = fa.AnnealedImportanceSampler(hf, target.log_prob, hmc, False, 2.0, M)
            pt, log_w = ais.sample_and_log_weights(B, eps0=eps0.to(DEV), noise_a=noise_p.to(DEV), noise_b=noise_e.to(DEV))
            info = ais._logging_info
            res[route] = (pt.x.clone(), pt.log_q.clone(), pt.log_p.clone(), log_w.clone(),
                          torch.tensor([info.ess_base, info.ess_ais, info.log_Z], dtype=torch.float64))
    finally:
        ops.set_option(_ops.OPT_FUSED_TAIL, 1)
    x, lq, lp, log_w, info = res[1]
    assert x.shape[0] == B - len(dead)
    print(f"MEASURE d | x {worst(x, opt.x):.2f} | log_w {worst(log_w, olw, M * RTOL):.2f}")
    assert close(x, opt.x, RTOL) and close(lq, opt.log_q, RTOL) and close(lp, opt.log_p, RTOL) and close(log_w, olw, M * RTOL)
    assert close(info, torch.tensor(list(oinfo), dtype=torch.float64), M * RTOL)
    for a, b in zip(res[1], res[0]):
        assert a.shape == b.shape and torch.equal(bits(a), bits(b))
