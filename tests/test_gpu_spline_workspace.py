"""Every spline entry point of the C ABI stays inside the workspace it asks for and gives the op layer's bits.

The calls go through ctypes with a workspace of EXACTLY fabhip_spline_workspace_bytes, 256-byte aligned, cut out of a larger
tensor with 4 KiB of a fixed int32 pattern in front and behind: a block the layout hands out beyond the reported size (or a
pointer computed differently from the size) lands in a guard.  The same inputs through torch.ops.fabhip.spline_* (scratch from
the caching allocator) must give the same outputs bit for bit."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

fa = pytest.importorskip("fab_torch_amd")
from fab_torch_amd import _lib, _ops      # noqa: E402
from oracle import spline as osp          # noqa: E402

DEV = "cuda"
GUARD = 4096                               # bytes in front of and behind the workspace
PATTERN = 0x5A5AA5A5                       # (as a float: 1.5e16, finite)
i32, i64, vp, sz = C.c_int32, C.c_int64, C.c_void_p, C.c_size_t


class SplineFlow(C.Structure):             # fabhip_spline_flow
    _fields_ = [("dim", i32), ("n_layers", i32), ("hidden", i32), ("precision", i32), ("packed", vp)]


# (dim, n_layers, hidden), circular coordinates, B, FABHIP_OPT_SPLINE_MFMA: the smallest shapes that reach every kernel family
# and a partial tile
CASES = [((6, 2, 64), (1, 4), 17, 0),            # 16x16x4 kernel, NTWM = 1, partial 16-row tile
         ((10, 2, 256), (3,), 9, 0),             # stream kernel, NCH = 1, partial 4-row block
         ((24, 2, 256), (2, 5), 9, 0),           # stream kernel, trimmed stream, NCH = 2
         ((10, 2, 256), (3,), 9, 16)]            # 16x16x4 kernel at NTWM = 4
_flows = {}


def flow_of(shape, circ):
    """A flow that has left its identity initialisation (the randomisation of test_gpu_spline.py), built once per shape."""
    if shape not in _flows:
        D, L, hidden = shape
        tb = torch.full((D,), 5.0)
        g = torch.Generator().manual_seed(D + L)
        tb[list(circ)] = math.pi / (0.5 + torch.rand(len(circ), generator=g))
        torch.manual_seed(D + L)
        of = osp.make_circular_coupled_flow(D, L, hidden, circ, tb, seed=D + L)
        osp.randomize(of, 0.4, D + L + 1)
        hf = fa.CircularCoupledRQSFlow(D, L, hidden, circ, tb, seed=D + L)
        hf._nf_model.load_state_dict(of.state_dict(), strict=True)
        hf = hf.to(DEV).requires_grad_(False)
        for f, _, _ in hf._structure():          # not the identity map: the conditioner's last Linear has left its zero init
            assert float(f.prqct.transform_net.final_layer.weight.abs().max()) > 0.1
        _flows[shape] = hf
    return _flows[shape]


class Guarded:
    """A workspace of exactly `nbytes`, 256-byte aligned, inside a tensor this test owns; the guards on both sides and the
    workspace itself start as PATTERN."""

    def __init__(self, nbytes):
        assert nbytes % 4 == 0
        self.buf = torch.empty((nbytes + 2 * GUARD + 256) // 4, dtype=torch.float32, device=DEV)
        self.words = self.buf.view(torch.int32)
        self.words.fill_(PATTERN)
        off = (-(self.buf.data_ptr() + GUARD)) % 256
        self.lo, self.n, self.nbytes = off // 4, nbytes // 4, nbytes
        self.ptr = vp(self.buf.data_ptr() + off + GUARD)
        assert self.ptr.value % 256 == 0

    def check(self, what):
        g = GUARD // 4
        front = self.words[self.lo: self.lo + g]
        behind = self.words[self.lo + g + self.n: self.lo + 2 * g + self.n]
        want = torch.full((g,), PATTERN, dtype=torch.int32, device=DEV)
        assert torch.equal(front, want), f"{what}: wrote in front of its workspace"
        assert torch.equal(behind, want), f"{what}: wrote behind the {self.nbytes} bytes it asked for"


def tape_written(tape, lay, L, B, n_id):
    """The words of a tape every call writes (include/fabhip.h: fabhip_spline_tape_layout): every block in full but dU, whose rows
    hold the identity positions' 25 cotangents only."""
    stride, o_du, udw = lay[1], lay[12], lay[15]
    out = []
    for l in range(L):
        t = tape[l * stride: (l + 1) * stride]
        out += [t[:o_du], t[o_du: o_du + B * udw].view(B, udw)[:, : n_id[l] * 25]]
    return out


@pytest.mark.parametrize("shape,circ,B,mfma", CASES)
def test_spline_entry_points_stay_inside_their_workspace_and_match_the_ops(shape, circ, B, mfma):
    D, L, hidden = shape
    hf = flow_of(shape, circ)
    lib, ops = _lib.load(), _ops.load()
    packed, *dims = hf.native()
    assert tuple(dims) == shape
    flow = SplineFlow(D, L, hidden, 0, vp(packed.data_ptr()))
    fl = C.byref(flow)
    wsb = lib.fabhip_spline_workspace_bytes
    wsb.restype, wsb.argtypes = sz, [i32, i32, i32, i64, i32]
    g = torch.Generator().manual_seed(7)
    x = (1.5 * torch.randn(B, D, generator=g)).to(DEV)
    u, eps = torch.rand(B, D, generator=g).to(DEV), torch.randn(B, D, generator=g).to(DEV)
    gx, gl = torch.randn(B, D, generator=g).to(DEV), torch.randn(B, generator=g).to(DEV)
    lay = (i64 * 16)()
    assert lib.fabhip_spline_tape_layout(D, L, hidden, B, lay) == 0
    lay = list(lay)
    n_id = [len(f.prqct.identity_features) for f, _, _ in hf._structure()]
    st = _lib.stream_ptr()
    p = lambda t: vp(t.data_ptr())               # noqa: E731
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)     # noqa: E731

    def same(what, got, want):
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), f"{what}: output {i} differs from the op's"

    with _ops.option(_ops.OPT_SPLINE_MFMA, mfma):
        for with_grad in (0, 1):                 # fabhip_spline_log_prob
            ws = Guarded(wsb(D, L, hidden, B, with_grad))
            lq, gr = new(B), new(B, D)
            rc = lib.fabhip_spline_log_prob(fl, p(x), p(lq), p(gr) if with_grad else None, i64(B), ws.ptr, sz(ws.nbytes), st)
            assert rc == 0
            ws.check(f"fabhip_spline_log_prob (with_grad = {with_grad})")
            lq_o, gr_o = ops.spline_logprob_grad(packed, D, L, hidden, x, bool(with_grad), 0)
            same("fabhip_spline_log_prob", [lq] + ([gr] if with_grad else []), [lq_o] + ([gr_o] if with_grad else []))

        ws = Guarded(wsb(D, L, hidden, B, 0))    # fabhip_spline_sample
        xs, lq = new(B, D), new(B)
        assert lib.fabhip_spline_sample(fl, p(u), p(eps), p(xs), p(lq), i64(B), ws.ptr, sz(ws.nbytes), st) == 0
        ws.check("fabhip_spline_sample")
        same("fabhip_spline_sample", [xs, lq], list(ops.spline_sample(packed, D, L, hidden, u, eps)))

        ws = Guarded(wsb(D, L, hidden, B, 1))    # fabhip_spline_log_prob_tape
        lq, gr, tape = new(B), new(B, D), new(lay[0])
        rc = lib.fabhip_spline_log_prob_tape(fl, p(x), p(lq), p(gr), i64(B), p(tape), i64(lay[0]), ws.ptr, sz(ws.nbytes), st)
        assert rc == 0
        ws.check("fabhip_spline_log_prob_tape")
        lq_o, gr_o, tape_o = ops.spline_logprob_tape(packed, D, L, hidden, x)
        same("fabhip_spline_log_prob_tape", [lq, gr] + tape_written(tape, lay, L, B, n_id),
             [lq_o, gr_o] + tape_written(tape_o, lay, L, B, n_id))

        ws = Guarded(wsb(D, L, hidden, B, 1))    # fabhip_spline_sample_vjp_tape
        v_x, v_base, t1, t2 = new(B, D), new(B, D), new(lay[0]), new(lay[0])
        rc = lib.fabhip_spline_sample_vjp_tape(fl, p(u), p(eps), p(gx), p(gl), p(v_x), p(v_base), i64(B), p(t1), p(t2), i64(lay[0]),
                                               ws.ptr, sz(ws.nbytes), st)
        assert rc == 0
        ws.check("fabhip_spline_sample_vjp_tape")
        t1_o, t2_o, vb_o = ops.spline_sample_vjp_tape(packed, D, L, hidden, u, eps, gx, gl)
        same("fabhip_spline_sample_vjp_tape", tape_written(t1, lay, L, B, n_id) + tape_written(t2, lay, L, B, n_id) + [v_base],
             tape_written(t1_o, lay, L, B, n_id) + tape_written(t2_o, lay, L, B, n_id) + [vb_o])
