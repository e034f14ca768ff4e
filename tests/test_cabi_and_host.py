"""CPU-only checks of the C-ABI library and of the host-side mirror (no GPU compute calls)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, close

import fab_torch_amd as fa
from fab_torch_amd import _lib
from oracle import ais as oais
from oracle import flow as oflow


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "fabhip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fabhip_[a-z_0-9]+)\s*\(", txt)))


def test_library_loads_and_exports_every_declared_symbol():
    lib = _lib.load()
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"libfabhip.so does not export {s}"
    assert sorted(_lib.SYMBOLS) == syms, "fab_torch_amd/_lib.py SYMBOLS out of sync with include/fabhip.h"
    assert lib.fabhip_version() >= 100
    assert b"workspace" in lib.fabhip_strerror(-4)


def test_build_sources_are_exactly_the_hip_files_of_csrc():
    """A unit that was added, renamed or deleted without its entry in _build.SOURCES fails here, not at link time on a GPU box."""
    from fab_torch_amd import _build
    present = sorted(f for f in os.listdir(_build.CSRC) if f.endswith(".hip"))
    assert len(set(_build.SOURCES)) == len(_build.SOURCES), "duplicate entry in _build.SOURCES"
    assert sorted(_build.SOURCES) == present


def test_abi_revision_and_developer_switches_without_gpu():
    """The ABI revision of the header, of both bindings and of the library agree; every developer switch of the header exists in
    the library with the default the header documents (the round-4 paths - one-launch phase tails, the in-kernel step-size rule,
    fused spline leapfrogs - are ON by default) and can be set / restored; an unknown key is rejected."""
    from fab_torch_amd import _ops
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "fabhip.h")).read()
    rev = int(re.search(r"#define FABHIP_ABI_VERSION (\d+)", txt).group(1))
    assert lib.fabhip_version() == rev == _lib.ABI_VERSION == _ops.ABI_VERSION
    keys = dict(re.findall(r"#define (FABHIP_OPT_[A-Z0-9_]+) (\d+)", txt))
    count = int(keys.pop("FABHIP_OPT_COUNT"))
    assert sorted(int(v) for v in keys.values()) == list(range(count)) == list(range(12))
    defaults = {"FABHIP_OPT_TILE_SHAPE": 0, "FABHIP_OPT_R4_STREAM": 2, "FABHIP_OPT_SCAN_VARIANT": 3, "FABHIP_OPT_SYSTEMATIC_VARIANT": 1,
                "FABHIP_OPT_SPLINE_STAGED": 0, "FABHIP_OPT_TIMELINE": 0, "FABHIP_OPT_SPLINE_MFMA": 0, "FABHIP_OPT_SPLINE_LEAP": 1,
                "FABHIP_OPT_FUSED_TAIL": 1, "FABHIP_OPT_ADAPT_FOLD": 1, "FABHIP_OPT_PGRAD": 1, "FABHIP_OPT_TAPE_TILES": 0}
    for name, key in keys.items():
        env = name.replace("FABHIP_OPT_", "FABHIP_").replace("TILE_SHAPE", "TILE")
        if env in os.environ:
            continue                                                   # (the library read the developer's override at load time)
        assert lib.fabhip_get_option(int(key)) == defaults[name], name
    assert (_ops.OPT_FUSED_TAIL, _ops.OPT_ADAPT_FOLD) == (int(keys["FABHIP_OPT_FUSED_TAIL"]), int(keys["FABHIP_OPT_ADAPT_FOLD"]))
    prev = lib.fabhip_set_option(int(keys["FABHIP_OPT_ADAPT_FOLD"]), 0)
    assert prev == 1 and lib.fabhip_get_option(int(keys["FABHIP_OPT_ADAPT_FOLD"])) == 0
    lib.fabhip_set_option(int(keys["FABHIP_OPT_ADAPT_FOLD"]), prev)
    assert lib.fabhip_set_option(count, 1) < 0 and lib.fabhip_get_option(-1) < 0
    assert {"FABHIP_AIS_INIT = 1", "FABHIP_AIS_FINISH = 2", "FABHIP_AIS_CONTINUE = 4"} <= set(re.findall(r"FABHIP_AIS_[A-Z]+ = \d", txt))


def test_geometry_queries_and_argument_validation_without_gpu():
    lib = _lib.load()
    n = lib.fabhip_flow_packed_floats(32, 10, 320)
    assert n > 10 * (16 * 320 + 320 * 320 + 320 * 32) * 2            # both orientations, padded
    assert lib.fabhip_flow_packed_floats(65, 2, 32) == -1              # dim beyond compiled limit
    assert lib.fabhip_flow_packed_floats(32, 2, 513) == -1
    assert lib.fabhip_hmc_workspace_bytes(1024, 32, 1) > 0
    assert lib.fabhip_hmc_workspace_bytes(1024, 32, 2) > lib.fabhip_hmc_workspace_bytes(1024, 32, 1)
    assert lib.fabhip_ais_workspace_bytes(1024, 32, 1) > lib.fabhip_hmc_workspace_bytes(1024, 32, 1)
    assert lib.fabhip_resample_workspace_bytes(1 << 20) >= 8 * (1 << 20)
    # null / bad arguments are rejected before any launch
    assert lib.fabhip_flow_log_prob(None, None, None, None, 4, None) == -1
    f = _lib.Flow(32, 2, 64, None)
    assert lib.fabhip_flow_sample(C.byref(f), None, None, None, 4, None) == -1
    assert lib.fabhip_gather_rows(None, None, None, 1, 1, None) == -1
    assert lib.fabhip_ess_logz(None, 4, None, 4.0, None, None, 0, None) == -1


def test_training_path_layout_matches_the_parameter_shapes_without_gpu():
    """fabhip_flow_grad_layout / _grad_views: the flat gradient image has exactly one slot per trainable scalar, in
    the shapes of the normflows-compatible parameters; tape sizes grow with the batch; bad arguments rejected."""
    lib = _lib.load()
    for D, K, nodes in [(32, 10, 10), (6, 8, 40), (5, 3, 4), (2, 4, 40)]:
        flow = fa.RealNVP(D, K, nodes)
        n = lib.fabhip_flow_grad_floats(D, K, D * nodes)
        tensors = flow._grad_tensors()
        assert n == sum(p.numel() for p in tensors) == sum(p.numel() for p in flow.parameters())
        views = flow._grad_views(torch.arange(n, dtype=torch.float32))
        assert [tuple(v.shape) for v in views] == [tuple(p.shape) for p in tensors]
        covered = torch.cat([v.reshape(-1) for v in views])
        assert torch.equal(covered, torch.arange(n, dtype=torch.float32))          # disjoint, complete, ordered
        t1 = lib.fabhip_flow_tape_bytes(D, K, D * nodes, 16)
        t2 = lib.fabhip_flow_tape_bytes(D, K, D * nodes, 17)
        assert 0 < t1 < t2 == lib.fabhip_flow_tape_bytes(D, K, D * nodes, 32)      # rows padded to the 16-chain tile
    assert lib.fabhip_flow_grad_floats(65, 2, 32) == -1
    assert lib.fabhip_flow_tape_bytes(65, 2, 32, 16) == 0
    assert lib.fabhip_flow_grad_layout(32, 10, 320, None) == -1
    f = _lib.Flow(32, 2, 64, None)
    assert lib.fabhip_flow_log_prob_tape(C.byref(f), None, None, None, 4, None, 0, None) == -1
    assert lib.fabhip_flow_param_grad(None, None, None, 0, None, 4, None, None) == -1
    assert lib.fabhip_adam_clip_step(None, None, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, None, 1.0, None, None, 0,
                                     None) == -1
    assert lib.fabhip_adam_workspace_bytes(1000) > 0


def test_train_step_plan_follows_the_tape_tile_option_without_gpu():
    """fabhip_train_step_plan (host-only): which tape kernel one fabhip_buffer_train_step call runs and whether the minibatch
    arithmetic is fused into its tail - the 8-chain tiles need D <= 32 and a hidden width padded to 256 / 320, the tail in addition
    FABHIP_OPT_TAPE_TILES = 0; bad arguments are rejected."""
    from fab_torch_amd import _ops
    lib = _lib.load()
    out = (C.c_int64 * 3)()
    key = _ops.OPT_TAPE_TILES
    prev = lib.fabhip_get_option(key)
    try:
        for mode in (0, 8, 16):
            lib.fabhip_set_option(key, mode)
            for (D, K, W), G in (((32, 10, 320), 5), ((20, 3, 320), 5), ((32, 2, 288), 5), ((32, 3, 256), 4), ((6, 3, 240), 4),
                                 ((31, 2, 186), 4)):
                assert lib.fabhip_train_step_plan(D, K, W, out) == 0
                assert list(out) == [16 if mode == 16 else 8, G, 1 if mode == 0 else 0], (mode, D, K, W, list(out))
            for D, K, W in ((6, 3, 30), (60, 3, 240), (33, 2, 264), (32, 2, 512), (32, 10, 128)):
                assert lib.fabhip_train_step_plan(D, K, W, out) == 0
                assert (out[0], out[2]) == (16, 0), (mode, D, K, W, list(out))
    finally:
        lib.fabhip_set_option(key, prev)
    assert lib.fabhip_train_step_plan(32, 10, 320, None) == -1
    assert lib.fabhip_train_step_plan(65, 2, 32, out) != 0


def test_anneal_coefficients_match_the_reference_formulas():
    lib = _lib.load()
    for beta in (0.0, 0.2, 1 / 3, 1.0):
        for alpha in (2.0, 0.5):
            a = _lib.Anneal()
            lib.fabhip_anneal_coefs(beta, alpha, 0, C.byref(a))
            assert a.c_q == np.float32((1 - beta) + beta * (1 - alpha)) and a.c_p == np.float32(beta * alpha)
            assert a.g_q == a.c_q and a.g_p == np.float32(2 * beta)       # base.py:116 quirk
            lib.fabhip_anneal_coefs(beta, alpha, 1, C.byref(a))
            assert a.c_q == np.float32(1 - beta) and a.c_p == np.float32(beta) and a.g_p == a.c_p


def test_beta_schedule_and_constructor_contracts():
    flow = fa.RealNVP(6, 2, 5)
    target = fa.ManyWellEnergy(6, use_gpu=False)
    hmc = fa.HamiltonianMonteCarlo(4, 6, flow.log_prob, target.log_prob, alpha=2.0, p_target=False, epsilon=1.0)
    assert hmc.uses_grad_info and set(hmc.state_dict()) == {"common_epsilon", "epsilons", "mass_vector"}
    np.testing.assert_allclose(hmc.epsilons.numpy(), 0.9) ; np.testing.assert_allclose(hmc.common_epsilon.numpy(), 0.1)
    met = fa.Metropolis(4, 6, flow.log_prob, target.log_prob, n_updates=3, alpha=2.0, max_step_size=5.0, min_step_size=1.0)
    assert not met.uses_grad_info and set(met.state_dict()) == {"noise_scalings"}
    np.testing.assert_allclose(met.noise_scalings[0].numpy(), [5.0, 3.0, 1.0])
    met.set_eval_mode(True)
    assert met.eval_mode is False           # the reference inverts the flag (metropolis.py:39-41)
    for M in (1, 4, 8):
        for sp in ("linear", "geometric"):
            ais = fa.AnnealedImportanceSampler(flow, target.log_prob, hmc, False, 2.0, M, sp)
            np.testing.assert_array_equal(ais.B_space.numpy(), oais.beta_schedule(M, sp).numpy())
    with pytest.raises(AssertionError):
        fa.AnnealedImportanceSampler(flow, target.log_prob, hmc, p_target=False, alpha=None)
    assert flow.event_shape == (6,)


def test_hot_path_fails_loudly_without_a_gpu():
    flow = fa.RealNVP(6, 2, 5).requires_grad_(False)
    x = torch.randn(4, 6)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.FabhipError):
            flow.log_prob(x)
        with pytest.raises(_lib.FabhipError):
            fa.ManyWellEnergy(6, use_gpu=False).log_prob(x)
        with pytest.raises(_lib.FabhipError):
            fa.effective_sample_size(torch.randn(8))


def test_state_dict_is_normflows_compatible_and_cpu_calls_fail_loudly():
    torch.manual_seed(0)
    nf = oflow.make_realnvp(6, 3, 5)
    oflow.randomize_last_layers(nf, 0.1, 1)
    flow = fa.RealNVP(6, 3, 5)
    assert set(flow._nf_model.state_dict()) == set(nf.state_dict())
    assert all(k.startswith("_nf_model.") for k in flow.state_dict())
    flow._nf_model.load_state_dict(nf.state_dict())
    from fab_torch_amd._lib import FabhipError
    x = torch.randn(16, 6)
    for call in (lambda: flow.log_prob(x), lambda: flow.sample_and_log_prob((16,)),
                 lambda: flow.sample_and_log_prob((16,), eps=torch.randn(16, 6))):
        with pytest.raises(FabhipError):              # parameters on the CPU / x on the CPU: no ATen fallback
            call()


def test_spline_flow_module_has_normflows_keys_and_fails_loudly_on_the_cpu():
    import math
    from oracle import spline as osp
    tb = torch.full((10,), 5.0); tb[[2, 7]] = math.pi
    of = osp.make_circular_coupled_flow(10, 4, 32, (2, 7), tb, seed=3)
    hf = fa.CircularCoupledRQSFlow(10, 4, 32, (2, 7), tb, seed=3)
    assert set(hf._nf_model.state_dict()) == set(of.state_dict())
    hf._nf_model.load_state_dict(of.state_dict())
    assert hf.event_shape == (10,)
    lib = _lib.load()
    assert lib.fabhip_spline_packed_floats(60, 12, 256) > 12 * 2 * (30 * 256 + 2 * 256 * 256 + 256 * 750)
    assert lib.fabhip_spline_packed_floats(65, 2, 64) == -1 and lib.fabhip_spline_packed_floats(60, 2, 257) == -1
    # training tape layout (host-only arithmetic): 3 [B][64] + 6 [B][Wp] + [B][NFP] + [B][64 * 25] per layer
    import ctypes
    lay = (ctypes.c_int64 * 16)()
    assert lib.fabhip_spline_tape_layout(60, 12, 256, 1024, lay) == 0
    Wp, NFP = lay[13], lay[14]
    assert (Wp, NFP, lay[15]) == (256, 768, 1600) and lay[1] == 1024 * (3 * 64 + 6 * Wp + NFP + 1600)
    assert lay[0] == 12 * lay[1] and list(lay[2:13]) == sorted(lay[2:13])
    assert lib.fabhip_spline_tape_layout(65, 2, 64, 8, lay) != 0
    with pytest.raises(_lib.FabhipError):
        hf.log_prob(torch.randn(4, 10))
    with pytest.raises(NotImplementedError):
        fa.CircularCoupledRQSFlow(10, 4, 32, (2, 7), tb, num_bins=4)


def test_workspace_sizes_are_the_recorded_ones():
    """Every *_workspace_bytes of the AIS and spline units against tests/golden/workspace_bytes.json (host-only functions).  The sizes come
    out of the carve functions that also hand the drivers their pointers: a block added to one layout shows up here."""
    import itertools
    import json
    lib = _lib.load()
    with open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")) as fh:
        rec = json.load(fh)
    i32, i64 = C.c_int32, C.c_int64
    realnvp = list(itertools.product([1, 15, 16, 17, 1024, 1152, 1153, 2048, 2049, 4096, 32769], [2, 6, 32, 33, 64], [1, 2, 5]))
    spline = [s + (B,) for s, B in itertools.product([(6, 4, 64), (60, 12, 256)], [16, 1000, 2048])]

    def ext_bytes(B, dim, n_inner, smc, moves):        # (only the switches of the modes are read: no device pointer needed)
        sa, mv = _lib.SmcArgs(enabled=smc), _lib.FlowMovesArgs(n_moves=moves)
        return lib.fabhip_ais_ext_workspace_bytes(B, dim, n_inner, C.byref(_lib.AisExt(C.pointer(sa), None, C.pointer(mv))))
    spline_ws = [s + (B, g) for s, B, g in itertools.product([(6, 4, 64), (24, 2, 256), (60, 12, 256)], [1, 16, 17, 1000, 2048], [0, 1])]
    grids = {"fabhip_hmc_workspace_bytes": ([i64, i32, i32], realnvp),
             "fabhip_spline_workspace_bytes": ([i32, i32, i32, i64, i32], spline_ws),
             "fabhip_metropolis_workspace_bytes": ([i64, i32, i32], realnvp),
             "fabhip_ais_workspace_bytes": ([i64, i32, i32], realnvp),
             "fabhip_ais_ext_workspace_bytes": (ext_bytes, [c + m for c in realnvp for m in ((0, 0), (0, 1), (1, 0), (1, 1))]),
             "fabhip_spline_hmc_workspace_bytes": ([i32, i32, i32, i64], spline),
             "fabhip_spline_ais_workspace_bytes": ([i32, i32, i32, i64], spline),
             "fabhip_smc_shard_workspace_bytes": ([i32, i64], list(itertools.product([1, 2, 64], [16, 2048])))}
    assert sorted(rec) == sorted(grids)
    for name, (argtypes, cases) in grids.items():
        fn = argtypes if callable(argtypes) else getattr(lib, name)
        if fn is not argtypes:
            fn.restype, fn.argtypes = C.c_size_t, argtypes
        want = {tuple(r[:-1]): r[-1] for r in rec[name]}
        assert sorted(want) == sorted(cases), f"{name}: the fixture does not hold the cases of this test"
        got = {c: fn(*c) for c in cases}
        assert got == want, {c: (got[c], want[c]) for c in cases if got[c] != want[c]}
    # no mode on, however it is said, is the plain size
    for c in realnvp[::7]:
        assert ext_bytes(*c, 0, 0) == lib.fabhip_ais_ext_workspace_bytes(*c, None) == lib.fabhip_ais_workspace_bytes(*c) == \
            lib.fabhip_ais_ext_workspace_bytes(*c, C.byref(_lib.AisExt()))


def test_spline_image_and_tape_layouts_are_the_recorded_ones():
    """fabhip_spline_packed_floats and all 16 words of fabhip_spline_tape_layout against tests/golden/spline_layout.json: the
    image and the tape are read by offset on both sides of the C ABI (spline_flow.py slices the tape), so a moved block shows here."""
    import itertools
    import json
    lib = _lib.load()
    with open(os.path.join(ROOT, "tests", "golden", "spline_layout.json")) as fh:
        rec = json.load(fh)
    shapes = [(6, 4, 64), (24, 2, 256), (60, 12, 256)]
    assert sorted(rec) == ["fabhip_spline_packed_floats", "fabhip_spline_tape_layout"]
    want = {tuple(r[:-1]): r[-1] for r in rec["fabhip_spline_packed_floats"]}
    assert sorted(want) == sorted(shapes)
    assert {s: lib.fabhip_spline_packed_floats(*s) for s in shapes} == want
    cases = [s + (B,) for s, B in itertools.product(shapes, [1, 17, 2048])]
    want = {tuple(r[:-1]): r[-1] for r in rec["fabhip_spline_tape_layout"]}
    assert sorted(want) == sorted(cases), "the fixture does not hold the cases of this test"
    lay = (C.c_int64 * 16)()
    for c in cases:
        assert lib.fabhip_spline_tape_layout(*c, lay) == 0
        assert list(lay) == want[c], (c, list(lay), want[c])


def test_ais_ext_struct_is_three_pointers_in_the_header_order():
    """fabhip_ais_ext (no fabhip_abi_sizes slot: three pointers, no padding to disagree on) against the ctypes mirror."""
    txt = open(os.path.join(ROOT, "include", "fabhip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} fabhip_ais_ext;", txt).group(1)
    fields = re.findall(r"const (fabhip_\w+)\* (\w+);", body)
    assert fields == [("fabhip_smc_args", "smc"), ("fabhip_defensive_args", "mix"), ("fabhip_flow_moves_args", "moves")]
    assert [n for n, _ in _lib.AisExt._fields_] == [n for _, n in fields]
    assert [t._type_ for _, t in _lib.AisExt._fields_] == [_lib.SmcArgs, _lib.DefensiveArgs, _lib.FlowMovesArgs]
    assert C.sizeof(_lib.AisExt) == 3 * C.sizeof(C.c_void_p)


def test_ais_run_ext_wants_the_share_of_every_mode_that_is_on_without_gpu():
    """fabhip_ais_run_ext on a workspace of fabhip_ais_workspace_bytes: FABHIP_ENOSPC with the SMC mode on and with one move, before
    anything is enqueued (the argument checks in front of the size check compare pointers with NULL only, so placeholders do).  A
    member that is present but off asks for nothing more: its size is the plain one here; the call itself runs in
    tests/test_gpu_ais_ext.py, since a call that passes the size check goes on to launch."""
    lib = _lib.load()
    B, D, M, n_inner, ENOSPC = 37, 6, 3, 2, -4
    some = 0x10000                                         # (never dereferenced: the call returns at the size check)
    a = _lib.AisArgs()
    a.flow = _lib.Flow(D, 3, 30, some)
    a.target = _lib.Target(_lib.TARGET_MANYWELL, D, -1.0, -6.0, 1.0, 0.0, 0, None, None)
    betas = (C.c_double * (M + 2))(0.0, 0.25, 0.5, 0.75, 1.0)
    a.B, a.M, a.betas, a.alpha, a.p_target, a.transition = B, M, betas, 2.0, 0, _lib.TRANSITION_HMC
    a.eps0 = a.noise_a = a.noise_b = a.step_state = a.common_epsilon = a.mass = a.log_w = a.n_valid = a.stats = some
    a.n_inner, a.L, a.max_grad, a.target_p_accept, a.tune = n_inner, 3, 1e3, 0.65, 1
    a.point = _lib.Point(some, some, some, some, some)
    a.workspace, a.workspace_bytes = some, lib.fabhip_ais_workspace_bytes(B, D, n_inner)
    smc, mv = _lib.SmcArgs(enabled=1, u=some), _lib.FlowMovesArgs(1, some, some, None)
    assert lib.fabhip_ais_run_ext(C.byref(a), C.byref(_lib.AisExt(C.pointer(smc), None, None)), None) == ENOSPC
    assert lib.fabhip_ais_run_ext(C.byref(a), C.byref(_lib.AisExt(None, None, C.pointer(mv))), None) == ENOSPC
    off = _lib.AisExt(C.pointer(_lib.SmcArgs(enabled=0)), C.pointer(_lib.DefensiveArgs(enabled=0)), C.pointer(_lib.FlowMovesArgs(0)))
    assert lib.fabhip_ais_ext_workspace_bytes(B, D, n_inner, C.byref(off)) == a.workspace_bytes
