"""The one ext form of the fused AIS call (include/fabhip.h: fabhip_ais_ext, fabhip_ais_run_ext / fabhip_ais_phase_ext; op
fabhip::ais_run_ext): with no mode on it is the plain call bit for bit, however "no mode" is said, and a call made in pieces with
two modes on equals the call made at once.

Shapes: D = 6, 3 layers, B = 37 (two 16-chain tiles, the second ragged), M = 3, n_inner = 2; all noise passed in.  Width 30 for
the C ABI; the op test runs at width 240 (padded to 256), the narrowest at which the library's own rule lets FABHIP_OPT_TILE_SHAPE
= 8 select the 8-chain tiles (they exist for padded widths 256 and 320 only; narrower flows fall back to the 16-chain tiles)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _lib, _ops                      # noqa: E402
from fab_torch_amd.ais import operator_slots                     # noqa: E402

DEV = "cuda"
D, K, NODES, NODES_WIDE, B, M, N_INNER, L = 6, 3, 5, 40, 37, 3, 2, 3
F32 = dict(dtype=torch.float32, device=DEV)
INIT, FINISH, CONTINUE = 1, 2, 4


def _sampler(hmc, nodes=NODES):
    torch.manual_seed(0)
    flow = fa.make_wrapped_normflow_realnvp(D, K, nodes, act_norm=False).to(DEV).requires_grad_(False)
    with torch.no_grad():
        for l1, l2, l3, aff in flow._layers():
            l3.weight.add_(0.01 * torch.randn_like(l3.weight))
    target = fa.ManyWellEnergy(D)
    if hmc:
        op = fa.HamiltonianMonteCarlo(M, D, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=0.1, n_outer=N_INNER,
                                      L=L).to(DEV)
    else:
        op = fa.Metropolis(M, D, flow.log_prob, target.log_prob, n_updates=N_INNER, alpha=2.0, p_target=False, max_step_size=0.4,
                           min_step_size=0.1, adjust_step_size=True).to(DEV)
    return flow, target, op, fa.AnnealedImportanceSampler(flow, target.log_prob, op, False, 2.0, M)


def _noise(hmc, k=0):
    g = torch.Generator().manual_seed(11)
    eps0 = torch.randn(B, D, generator=g)
    na = torch.randn(M, N_INNER, B, D, generator=g)
    nb = torch.empty(M, N_INNER, B).exponential_(1.0, generator=g) if hmc else torch.rand(M, N_INNER, B, generator=g)
    ng = torch.randn(M, max(k, 1), B, D, generator=g)
    nh = torch.empty(M, max(k, 1), B).exponential_(1.0, generator=g)
    nr = torch.rand(M, generator=g, dtype=torch.float64)
    return tuple(t.to(DEV) for t in (eps0, na, nb, ng, nh, nr))


def _step_state(op):
    return (op.epsilons, op.common_epsilon) if isinstance(op, fa.HamiltonianMonteCarlo) else (op.noise_scalings,)


# ---- the op ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["hmc-4", "hmc-8", "hmc-16", "metropolis"])
def test_ais_run_ext_with_every_mode_off_is_ais_run(route):
    hmc = route != "metropolis"
    eps0, na, nb, _, _, _ = _noise(hmc)
    ops = _ops.load()
    runs = []
    with _ops.option(_ops.OPT_TILE_SHAPE, int(route[4:]) if hmc else 0):
        for call in (ops.ais_run, ops.ais_run_ext):
            flow, target, op, ais = _sampler(hmc, NODES_WIDE)
            kind, slots = operator_slots(op)
            out = call(*ais._call_head(flow, target, kind), eps0, na, nb, *slots, True, _ops.precision_of(flow))
            runs.append((list(out), [t.clone() for t in _step_state(op)]))
    (plain, state0), (ext, state1) = runs
    assert len(plain) == 10 and len(ext) == 15
    for i, (u, v) in enumerate(zip(plain, ext)):
        assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v), f"{route}: output {i} differs"
    assert all(torch.equal(u, v) for u, v in zip(state0, state1)), f"{route}: the step-size state differs"
    assert int(plain[6][0]) > 0 and all(t.numel() == 0 for t in ext[10:])
    assert [t.dtype for t in ext[10:]] == [torch.int32, torch.float32, torch.int32, torch.float32, torch.float32]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
class _CCall:
    """fabhip_ais_args over tensors of its own (HMC), the operator's initial step-size state, a workspace of `ext_bytes`."""

    def __init__(self, noise, ext_bytes):
        flow, target, op, ais = _sampler(True)
        self.keep = (flow, target, op, noise)
        eps0, na, nb = noise[:3]
        packed, _, _, W = flow.native()
        a = self.a = _lib.AisArgs()
        a.flow = _lib.Flow(D, K, W, packed.data_ptr())
        kind, prm, _, _ = target.native_target()
        a.target = _lib.Target(kind, D, prm[0], prm[1], prm[2], prm[3], 0, None, None)
        self.betas = (C.c_double * (M + 2))(*[float(b) for b in ais.B_space])
        a.B, a.M, a.betas, a.alpha, a.p_target, a.transition = B, M, self.betas, 2.0, 0, _lib.TRANSITION_HMC
        a.eps0, a.noise_a, a.noise_b = eps0.data_ptr(), na.data_ptr(), nb.data_ptr()
        self.step0 = (op.epsilons.clone(), op.common_epsilon.clone())
        self.step = (op.epsilons.clone(), op.common_epsilon.clone())
        a.step_state, a.common_epsilon, a.mass = self.step[0].data_ptr(), self.step[1].data_ptr(), op.mass_vector.data_ptr()
        a.n_inner, a.L, a.max_grad, a.target_p_accept, a.tune = N_INNER, L, op.max_grad, op.target_p_accept, 1
        self.out = [torch.empty(B, D, **F32), torch.empty(B, **F32), torch.empty(B, **F32), torch.empty(B, D, **F32),
                    torch.empty(B, D, **F32), torch.empty(B, **F32), torch.zeros(2, dtype=torch.int32, device=DEV),
                    torch.zeros(16, **F32)]
        x, lq, lp, gq, gp, lw, nv, st = self.out
        a.point = _lib.Point(x.data_ptr(), lq.data_ptr(), lp.data_ptr(), gq.data_ptr(), gp.data_ptr())
        a.log_w, a.n_valid, a.stats = lw.data_ptr(), nv.data_ptr(), st.data_ptr()
        self.ws = torch.empty(ext_bytes + 256, dtype=torch.uint8, device=DEV)
        a.workspace, a.workspace_bytes = (self.ws.data_ptr() + 255) // 256 * 256, ext_bytes
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def reset(self):
        for t, t0 in zip(self.step, self.step0):
            t.copy_(t0)
        for t in self.out:
            t.zero_()

    def result(self, *more):
        torch.cuda.synchronize()
        return [t.clone() for t in (*self.out, *self.step, *more)]


def test_c_abi_null_ext_empty_ext_and_members_that_are_off_are_fabhip_ais_run():
    """(The last form on a workspace of the plain size: a member that is present but off must not ask for its share.)"""
    lib = _lib.load()
    c = _CCall(_noise(True), lib.fabhip_ais_workspace_bytes(B, D, N_INNER))
    a, results = C.byref(c.a), []
    off = _lib.AisExt(C.pointer(_lib.SmcArgs(enabled=0)), C.pointer(_lib.DefensiveArgs(enabled=0)), C.pointer(_lib.FlowMovesArgs(0)))
    for call in (lambda: lib.fabhip_ais_run(a, c.stream), lambda: lib.fabhip_ais_run_ext(a, None, c.stream),
                 lambda: lib.fabhip_ais_run_ext(a, C.byref(_lib.AisExt(None, None, None)), c.stream),
                 lambda: lib.fabhip_ais_run_ext(a, C.byref(off), c.stream)):
        c.reset()
        _lib.check(call(), "fused AIS call")
        results.append(c.result())
    assert int(results[0][6][1]) > 0 and not torch.equal(results[0][8], c.step0[0])      # (chains survived, the step sizes moved)
    for other in results[1:]:
        assert all(torch.equal(u, v) for u, v in zip(results[0], other))


def test_c_abi_phases_with_smc_and_moves_equal_the_whole_call():
    lib = _lib.load()
    k = 2
    noise = _noise(True, k)
    ng, nh, nr = noise[3:]
    resampled, anc = torch.full((M,), -1, dtype=torch.int32, device=DEV), torch.full((M, B), -1, dtype=torch.int32, device=DEV)
    ess, lw_pre, fracs = torch.full((M,), -1.0, **F32), torch.full((M, B), -1.0, **F32), torch.full((M, k), -1.0, **F32)
    records = (resampled, ess, anc, lw_pre, fracs)
    smc = _lib.SmcArgs(1, 0, 0.9, nr.data_ptr(), resampled.data_ptr(), ess.data_ptr(), anc.data_ptr(), lw_pre.data_ptr(), 0)
    mv = _lib.FlowMovesArgs(k, ng.data_ptr(), nh.data_ptr(), fracs.data_ptr())
    ext = C.byref(_lib.AisExt(C.pointer(smc), None, C.pointer(mv)))
    c = _CCall(noise, lib.fabhip_ais_ext_workspace_bytes(B, D, N_INNER, ext))
    a = C.byref(c.a)
    _lib.check(lib.fabhip_ais_run_ext(a, ext, c.stream), "ais_run_ext")
    whole = c.result(*records)
    assert int(whole[6][1]) > 0 and bool(whole[10].any()) and float(whole[14].min()) >= 0.0     # (a resampling fired, the moves ran)
    c.reset()
    for t in records:
        t.fill_(-1)
    _lib.check(lib.fabhip_ais_phase_ext(a, ext, INIT, 1, 0, None, c.stream), "INIT")
    for j in range(1, M + 1):
        _lib.check(lib.fabhip_ais_phase_ext(a, ext, CONTINUE, j, j, None, c.stream), f"transition {j}")
    _lib.check(lib.fabhip_ais_phase_ext(a, ext, CONTINUE | FINISH, 1, 0, None, c.stream), "FINISH")
    pieces = c.result(*records)
    for i, (u, v) in enumerate(zip(whole, pieces)):
        assert torch.equal(u, v), f"array {i} differs between the whole call and its pieces"
