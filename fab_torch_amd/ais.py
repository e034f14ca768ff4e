"""AnnealedImportanceSampler with the reference's interface (fab/sampling_methods/ais.py:20-213).

`sample_and_log_weights(batch_size)` is ONE custom-op call (torch.ops.fabhip.ais_run -> fabhip_ais_run): flow sample, point creation,
initial log-weights, NaN/inf compaction, M fused transitions with log-weight accumulation, final
compaction and ESS / log Z — enqueued back-to-back on the current HIP stream with a single small
device->host read at the end (row counts + logging scalars)."""
from collections import namedtuple
from typing import Any, Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _ops
from .defensive import DefensiveMixtureDistribution
from .flow import RealNVP
from .point import Point
from .targets import _NativeTarget
from .transition_operators import (HamiltonianMonteCarlo, Metropolis, TransitionOperator, create_point,
                                   create_point_generic, _owner, _owner_or_none)


class NoValidPoints(Exception):
    """The reference's `Exception("No valid points generated in sampling the chain init / end")` (ais.py:202-204, 211) as a class of
    its own - same message, still an `Exception` for callers written against the reference - so that the sharded sampler can tell
    an empty shard from any other failure (it matched the message text of a bare Exception).  `phase`: "init" / "end"."""

    def __init__(self, phase: str):
        super().__init__(f"No valid points generated in sampling the chain {phase}")
        self.phase = phase


class LoggingInfo(NamedTuple):
    ess_base: float
    ess_ais: float
    log_Z: float


def check_noise_r(noise_r: torch.Tensor, M: int) -> torch.Tensor:
    """The uniforms of the resampling steps: ONE float64 in [0, 1) per transition, `[M]` (the device clamps a value outside the
    range to 0; the host does not read the values)."""
    if not torch.is_tensor(noise_r) or noise_r.dtype != torch.float64 or tuple(noise_r.shape) != (int(M),):
        got = (tuple(noise_r.shape), noise_r.dtype) if torch.is_tensor(noise_r) else type(noise_r).__name__
        raise _ops.FabhipError(f"noise_r must be a float64 tensor of shape [{int(M)}] (one uniform per transition), got {got}")
    return noise_r.contiguous()


# The transition operator's segment of the fused ops' argument lists, in schema order (ais_run / ais_run_ext / spline_ais_run
# take it whole; ais_phase takes the four logging slots apart, behind the state tensors).
OperatorSlots = namedtuple("OperatorSlots", "step_state common_epsilon mass n_inner L max_grad target_p_accept tune "
                                            "p_accept_first p_accept_last avg_distance_first avg_distance_last")


def operator_slots(op) -> Tuple[int, OperatorSlots]:
    """(transition kind, the operator's slots) of this package's HMC / Metropolis."""
    if isinstance(op, HamiltonianMonteCarlo):
        return _ops.TRANSITION_HMC, OperatorSlots(
            op.epsilons, op.common_epsilon, op.mass_vector, op.n_outer, op.L, float(op.max_grad), float(op.target_p_accept),
            not op.eval_mode, op._p_accept_first, op._p_accept_last, op._dist_first, op._dist_last)
    if isinstance(op, Metropolis):
        return _ops.TRANSITION_METROPOLIS, OperatorSlots(
            op.noise_scalings, None, None, op.n_updates, 0, 0.0, float(op.target_prob_accept),
            bool(op.adjust_step_size and not op.eval_mode), None, None, None, None)
    raise _ops.FabhipError("transition_operator must be a fab_torch_amd HamiltonianMonteCarlo / Metropolis")


RESAMPLE_METHODS = {"systematic": 0, "stratified": 1}      # FABHIP_SMC_SYSTEMATIC / FABHIP_SMC_STRATIFIED


def check_resample_method(method) -> str:
    if not isinstance(method, str) or method not in RESAMPLE_METHODS:
        raise _ops.FabhipError(f"resample_method must be one of {sorted(RESAMPLE_METHODS)} (got {method!r})")
    return method


def _check_threshold(tau):
    if tau is None:
        return None
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or tau != tau:
        raise _ops.FabhipError(f"resample_threshold must be None (plain AIS) or a number (ESS fraction), got {tau!r}")
    return float(tau)


def check_n_flow_moves(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) < 0:
        raise _ops.FabhipError(f"n_flow_moves must be a non-negative integer: the flow-proposal moves in front of every "
                               f"transition (got {k!r})")
    return int(k)


def check_move_noise(noise_g, noise_h, M: int, k: int, B: int, D: int):
    """The draws of the flow-proposal moves: noise_g [M, k, B, D] normals (the proposals' base noise) and noise_h [M, k, B]
    standard exponentials, float32."""
    for name, t, shape in (("noise_g", noise_g, (M, k, B, D)), ("noise_h", noise_h, (M, k, B))):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape:
            got = (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__
            raise _ops.FabhipError(f"{name} must be a float32 tensor of shape {list(shape)} "
                                   f"([M, n_flow_moves, batch{', dim' if name == 'noise_g' else ''}]), got {got}")
    return noise_g.contiguous(), noise_h.contiguous()


def check_schedule(values, M: int, what: str = "distribution_spacing_type") -> torch.Tensor:
    """A caller's annealing schedule as the float64 `B_space` tensor: M + 2 finite, non-decreasing values from 0 to 1 (repeated
    entries are legal: the increment of such a step is skipped)."""
    if torch.is_tensor(values):
        if values.dtype != torch.float64:
            raise _ops.FabhipError(f"{what}: a schedule given as a tensor must be float64 (got {values.dtype})")
        b = values.detach().cpu().numpy()
    else:
        try:
            b = np.asarray(values, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise _ops.FabhipError(f"{what} must be 'linear', 'geometric', 'adaptive' or a sequence of {int(M) + 2} numbers "
                                   f"(got {values!r})") from e
    if b.shape != (int(M) + 2,):
        raise _ops.FabhipError(f"{what}: a schedule needs n_intermediate_distributions + 2 = {int(M) + 2} values, got shape "
                               f"{tuple(b.shape)}")
    if not np.isfinite(b).all() or b[0] != 0.0 or b[-1] != 1.0 or (np.diff(b) < 0).any():
        raise _ops.FabhipError(f"{what}: a schedule must be finite and non-decreasing, start at 0 and end at 1 (got {b.tolist()})")
    return torch.tensor(b, dtype=torch.float64)


def check_ess_decay(rho) -> float:
    if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not 0.0 < float(rho) < 1.0:
        raise _ops.FabhipError(f"ess_decay must be a number in (0, 1): the fraction of the current ESS a step keeps (got {rho!r})")
    return float(rho)


class AdaptiveDecision(NamedTuple):
    """One decision of an adaptive schedule: made after transition `step` (0: after the chain initialisation) at `beta`."""
    step: int
    beta: float
    beta_next: float          # the decision's own value (a forced schedule may have used another)
    ess0: float
    ess_choice: float
    evaluations: int
    floor: bool
    inputs: Optional[tuple]   # (log_w, log_q, log_p) as the kernel saw them (`trace=True`), else None


NEXT_BETA_ITERS = 24          # K of fabhip_next_beta: the schedule is resolved to (1 - beta) 2^-24


class AnnealedImportanceSampler:
    """`distribution_spacing_type`: "linear" / "geometric" (the reference's), a schedule of the caller's (sequence, array or
    float64 tensor of M + 2 non-decreasing values from 0 to 1), or "adaptive": every temperature is chosen on the device from
    the weights (fabhip_next_beta: the largest step that keeps `ess_decay` of the current ESS, by bisection), the call is
    stepped transition by transition with one 32-byte read each, `last_betas` holds the schedule the call chose and `B_space`
    the linear one as a nominal value.

    `resample_threshold` (SMC mode, default None = plain AIS): before every transition the ESS of the current log-weights is
    computed on the device; below the threshold the chains are resampled in proportion to their weights (systematic, on the
    fixed-point CDF of `resample_systematic`) and continue with equal weights whose logsumexp is unchanged, so `log_Z`, the FAB
    loss and the buffer see an ordinary `(point, log_w)`.  > 1: before every transition; 0: never (the decision still runs).
    `resample_method` ("systematic", the default, or "stratified") chooses the ancestors of a resampling step: "stratified" draws
    one offset per stratum (a hash of the transition's uniform and the stratum number; include/fabhip.h:
    fabhip_resample_stratified) instead of one for all of them - unbiased like the systematic scheme, but with a variance that is
    never above multinomial resampling's whatever the order of the chains.  The decision, `noise_r` and its draws are the same
    for both; without `resample_threshold` the setting is inert.

    `n_flow_moves` (default 0: none): flow-proposal independence moves in front of every transition - step j runs [resampling
    step,] n_flow_moves x (x' = a fresh sample of the flow, accepted with min(1, [pi_j(x') / q(x')] / [pi_j(x) / q(x)])), then
    transition j: the one global move of the sampler (definition: tests/flow_move_spec.py; fabhip_flow_move).  The moves leave
    pi_j invariant, so the weights are what they were; `last_flow_moves` holds the acceptance fractions [M, n_flow_moves] of the
    last call (a device tensor).  RealNVP base and native target only."""

    def __init__(self, base_distribution, target_log_prob, transition_operator: TransitionOperator,
                 p_target: bool, alpha: Optional[float] = None, n_intermediate_distributions: int = 1,
                 distribution_spacing_type="linear", resample_threshold: Optional[float] = None,
                 resample_method: str = "systematic", ess_decay: float = 0.7, n_flow_moves: int = 0):
        if not p_target:
            assert alpha is not None, "Must specify alpha if AIS target is not p."
        self.n_flow_moves = n_flow_moves
        self.last_flow_moves = None       # float32 [M, n_flow_moves] on the device: acceptance fractions of the last call
        self.resample_threshold = resample_threshold
        self.resample_method = resample_method
        self.ess_decay = ess_decay        # adaptive schedules only: the fraction of the current ESS a step keeps
        self.last_betas = None            # float64 [M + 2]: the schedule the last adaptive call chose
        self.last_adaptive = None         # its decisions (AdaptiveDecision)
        self.last_smc = None              # (resampled [M], ess [M], ancestors [M, B], log_w_pre [M, B]) of the last fused call
        self.base_distribution = base_distribution
        self.target_log_prob = target_log_prob
        self.transition_operator = transition_operator
        self.p_target = p_target
        self.alpha = alpha
        self.n_intermediate_distributions = n_intermediate_distributions
        self.distribution_spacing_type = distribution_spacing_type
        self.B_space = self.setup_distribution_spacing(distribution_spacing_type, n_intermediate_distributions)
        self._logging_info: LoggingInfo
        self._last_stats = None

    @property
    def resample_threshold(self) -> Optional[float]:
        return self.__dict__.get("_resample_threshold")      # (None for a sampler restored from a state that predates the setting)

    @resample_threshold.setter
    def resample_threshold(self, tau):
        self.__dict__["_resample_threshold"] = _check_threshold(tau)

    @property
    def n_flow_moves(self) -> int:
        return self.__dict__.get("_n_flow_moves", 0)          # (0 for a sampler restored from a state that predates the setting)

    @n_flow_moves.setter
    def n_flow_moves(self, k):
        self.__dict__["_n_flow_moves"] = check_n_flow_moves(k)

    def _refuse_flow_moves(self, what: str):
        if self.n_flow_moves > 0:
            raise _ops.FabhipError(f"n_flow_moves={self.n_flow_moves} (flow-proposal moves) is not available for {what}: set "
                                   "n_flow_moves=0, or use a RealNVP base distribution with a native target")

    def _refuse_flow_move_routes(self):
        """The routes the flow-proposal moves do not run on, refused by name before any op is reached."""
        if self.n_flow_moves == 0:
            return
        if self._spline_parts() is not None:
            self._refuse_flow_moves("the fused spline-flow call")
        if isinstance(self.base_distribution, DefensiveMixtureDistribution):
            self._refuse_flow_moves("a DefensiveMixtureDistribution base (the proposal would have to be the mixture)")
        if not self.is_native:
            self._refuse_flow_moves("the generic path (plug-in base distribution / target / transition operator)")

    @property
    def resample_method(self) -> str:
        return self.__dict__.get("_resample_method", "systematic")   # (a sampler restored from a state that predates the setting)

    @resample_method.setter
    def resample_method(self, method):
        self.__dict__["_resample_method"] = check_resample_method(method)

    @property
    def ess_decay(self) -> float:
        return self.__dict__.get("_ess_decay", 0.7)

    @ess_decay.setter
    def ess_decay(self, rho):
        self.__dict__["_ess_decay"] = check_ess_decay(rho)

    @property
    def adaptive(self) -> bool:
        t = self.__dict__.get("distribution_spacing_type")
        return isinstance(t, str) and t == "adaptive"

    def _refuse_adaptive(self, what: str, instead: str):
        if self.adaptive:
            raise _ops.FabhipError(f"distribution_spacing_type='adaptive' is not available for {what}: {instead}")

    def _refuse_adaptive_routes(self):
        """The routes an adaptive schedule does not run on, refused by name before any op is reached."""
        if not self.adaptive:
            return
        fixed = "set distribution_spacing_type to 'linear', 'geometric' or a schedule of your own"
        if self._spline_parts() is not None:
            self._refuse_adaptive("the fused spline-flow call", fixed + " (the last_betas of a RealNVP run, for instance)")
        if isinstance(self.base_distribution, DefensiveMixtureDistribution):
            self._refuse_adaptive("a DefensiveMixtureDistribution base (the call made in pieces refuses the mixture)", fixed)
        if not self.is_native:
            self._refuse_adaptive("the generic path (plug-in base distribution / target / transition operator)", fixed)

    def _refuse_resampling(self, what: str):
        if self.resample_threshold is not None:
            raise _ops.FabhipError(f"resample_threshold={self.resample_threshold} (SMC mode) is not available for {what}: "
                                   "set resample_threshold=None, or use a RealNVP / generic base distribution")

    def get_logging_info(self) -> Dict[str, Any]:
        info = self._logging_info._asdict()
        if self.resample_threshold is not None and self.__dict__.get("_smc_info") is not None:
            info.update(self._smc_info)                     # n_resampled, ess_min_in_chain of the last logged call
        if self.adaptive and self.__dict__.get("_adaptive_info") is not None:
            info.update(self._adaptive_info)                # beta_1, n_steps_to_beta_one, n_bisect_floor of the last call
        if self.n_flow_moves > 0 and self.__dict__.get("_flow_move_info") is not None:
            info.update(self._flow_move_info)               # flow_move_p_accept_dist0 / dist{M-1} of the last logged call
        info.update(self.transition_operator.get_logging_info())
        return info

    def setup_distribution_spacing(self, distribution_spacing_type, n_intermediate_distributions: int
                                   ) -> torch.Tensor:
        assert n_intermediate_distributions > 0
        if not isinstance(distribution_spacing_type, str):                       # a schedule of the caller's
            return check_schedule(distribution_spacing_type, n_intermediate_distributions)
        if distribution_spacing_type == "geometric":
            n_lin = int(n_intermediate_distributions / 4)
            n_geo = n_intermediate_distributions - n_lin - 1
            B_space = np.concatenate([np.linspace(0, 0.01, n_lin + 2)[:-1], np.geomspace(0.01, 1, n_geo + 2)])
        elif distribution_spacing_type in ("linear", "adaptive"):                # (adaptive: the nominal value of B_space)
            B_space = np.linspace(0.0, 1.0, n_intermediate_distributions + 2)
        else:
            raise Exception(f"distribution spacing incorrectly specified: '{distribution_spacing_type}',"
                            f"options are 'geometric', 'linear', 'adaptive' or a sequence of M + 2 values")
        assert B_space.shape == (self.n_intermediate_distributions + 2,)
        return torch.tensor(B_space)

    # ---------------------------------------------------------------------------------------------
    def _mixture(self) -> Optional[DefensiveMixtureDistribution]:
        """The defensive mixture this sampler draws from when the fused call applies to it (a RealNVP inside), else None."""
        base = self.base_distribution
        return base if isinstance(base, DefensiveMixtureDistribution) and base.is_native else None

    def _refuse_mixture(self, what: str):
        if self._mixture() is not None:
            raise _ops.FabhipError(f"a DefensiveMixtureDistribution base is not available for {what}: the mixture runs through "
                                   "the one-op fused call (fabhip::ais_run_ext) only")

    def _native_parts(self) -> Tuple[RealNVP, _NativeTarget]:
        """(RealNVP, native target) of the fused call; with a defensive mixture as base distribution the RealNVP inside it
        (`_mixture()` tells the two apart: the mixture's call is ais_run_ext with its mix group)."""
        mix = self._mixture()
        flow = mix.flow if mix is not None else self.base_distribution
        if not isinstance(flow, RealNVP):
            raise _ops.FabhipError("base_distribution must be a fab_torch_amd RealNVP for the HIP path "
                                   "(no generic / CPU fallback)")
        target = _owner(self.target_log_prob, _NativeTarget, "target_log_prob")
        return flow, target

    def _spline_parts(self):
        """(spline flow, native target) when the fused SPLINE call applies: this package's spline flow as base
        distribution, a native target, HMC transitions (fabhip_spline_ais_run); else None."""
        from .spline_flow import CircularCoupledRQSFlow
        op = self.transition_operator
        if not isinstance(self.base_distribution, CircularCoupledRQSFlow) or not isinstance(op, HamiltonianMonteCarlo) \
                or op.force_stepwise:
            return None
        target = _owner_or_none(self.target_log_prob, _NativeTarget)
        return (self.base_distribution, target) if target is not None else None

    def _run_spline(self, batch_size: int, eps0=None, noise_a=None, noise_b=None, want_base: bool = False, u0=None):
        """`run` for the spline family: ONE op call (torch.ops.fabhip.spline_ais_run).  `eps0` / `u0` [B, D]: the normal /
        uniform draws of the flow's base sample."""
        self._refuse_resampling("the fused spline-flow call")
        self._refuse_adaptive_routes()
        self._refuse_flow_move_routes()
        flow, target = self._spline_parts()
        op = self.transition_operator
        head = self._call_head(flow, target, _ops.TRANSITION_HMC)[:-1]       # (HMC only: the spline op has no transition slot)
        dev = flow._tail_bound.device
        B, D, M = int(batch_size), flow.dim, self.n_intermediate_distributions
        f32 = dict(dtype=torch.float32, device=dev)
        u0 = torch.rand((B, D), **f32) if u0 is None else u0.contiguous()
        eps0 = torch.randn((B, D), **f32) if eps0 is None else eps0.contiguous()
        noise_a = torch.randn((M, op.n_outer, B, D), **f32) if noise_a is None else noise_a.contiguous()
        noise_b = torch.empty((M, op.n_outer, B), **f32).exponential_(1.0) if noise_b is None else noise_b.contiguous()
        out = _ops.load().spline_ais_run(*head, u0, eps0, noise_a, noise_b, *operator_slots(op)[1], bool(want_base),
                                         _ops.precision_of(flow))
        x, lq, lp, gq, gp, log_w, n_valid, stats, base_x, base_lw = out
        return Point(x, lq, lp, gq, gp), log_w, n_valid, stats, base_x, base_lw

    def run(self, batch_size: int, eps0=None, noise_a=None, noise_b=None, want_base: bool = False, u0=None, noise_r=None,
            trace: bool = False, sel=None, force_betas=None, noise_g=None, noise_h=None):
        """(`noise_g` [M, k, B, D] normals / `noise_h` [M, k, B] standard exponentials, float32: the draws of the k =
        n_flow_moves flow-proposal moves in front of every transition; absent: drawn on the device after noise_a / noise_b, g
        before h.  An error with n_flow_moves == 0.)
        (`force_betas` [M + 2], adaptive schedules only: the call runs on this schedule; the decisions still run and are
        recorded in `last_adaptive` - with `trace` together with the log_w, log_q, log_p each of them saw.)
        (`sel` [B] uniforms in [0, 1): the branch draws of a DefensiveMixtureDistribution base - chain i starts from the flow iff
        sel_i < sigmoid(mixture_logit); absent: drawn on the device after eps0 and before the transition noise.)
        (`noise_r` [M] float64: the uniforms of the resampling steps, SMC mode only; `trace`: keep the ancestors and the
        log-weights every decision saw in `last_smc`.)
        (`u0` [B, D]: the uniform base draws of the SPLINE flow; an error for any other base distribution.)
        Enqueue one AIS call; returns device tensors (Point fields sized [batch_size], log_w, n_valid[2],
        stats[16], base_x, base_log_w) without synchronising.  `want_base`: also return the chains' starting points
        after the "chain init" filtering and their log p - log q (generate_eval_data, ais.py:152-166)."""
        self._refuse_adaptive_routes()
        self._refuse_flow_move_routes()
        k_moves = self.n_flow_moves
        if (noise_g is not None or noise_h is not None) and k_moves == 0:
            raise _ops.FabhipError("noise_g / noise_h belong to the flow-proposal moves: set n_flow_moves first")
        if (noise_g is None) != (noise_h is None):
            raise _ops.FabhipError("pass both noise_g and noise_h (the draws of the flow-proposal moves) or neither")
        if force_betas is not None and not self.adaptive:
            raise _ops.FabhipError("force_betas belongs to distribution_spacing_type='adaptive'; a fixed schedule is passed as "
                                   "distribution_spacing_type itself")
        if self._spline_parts() is not None:
            return self._run_spline(batch_size, eps0, noise_a, noise_b, want_base, u0=u0)
        if u0 is not None:
            raise _ops.FabhipError("u0 (uniform base draws) belongs to the fused spline-flow call; a RealNVP takes eps0 only")
        if self.adaptive:
            if sel is not None:
                raise _ops.FabhipError("sel (branch uniforms) belongs to a DefensiveMixtureDistribution base distribution")
            return self._run_adaptive(batch_size, eps0, noise_a, noise_b, want_base, noise_r, trace, force_betas, noise_g,
                                      noise_h)
        ops = _ops.load()
        flow, target = self._native_parts()
        kind, slots = operator_slots(self.transition_operator)
        head = self._call_head(flow, target, kind)
        dev = flow._nf_model.q0.loc.device
        B, D, M = int(batch_size), flow.dim, self.n_intermediate_distributions
        hmc, n_inner = kind == _ops.TRANSITION_HMC, slots.n_inner
        f32 = dict(dtype=torch.float32, device=dev)
        eps0 = torch.randn((B, D), **f32) if eps0 is None else eps0.contiguous()
        # (both absent: drawn inside the op, in this order, AFTER the chain initialisation is enqueued - the device works meanwhile)
        if noise_a is not None or noise_b is not None:
            if noise_a is None:
                noise_a = torch.randn((M, n_inner, B, D), **f32)
            if noise_b is None:
                noise_b = (torch.empty((M, n_inner, B), **f32).exponential_(1.0) if hmc
                           else torch.rand((M, n_inner, B), **f32))
            noise_a, noise_b = noise_a.contiguous(), noise_b.contiguous()
            assert noise_a.shape == (M, n_inner, B, D) and noise_b.shape == (M, n_inner, B)
        tau = self.resample_threshold
        if noise_r is not None:
            if tau is None:
                raise _ops.FabhipError("noise_r belongs to the SMC mode: set resample_threshold first")
            noise_r = check_noise_r(noise_r, M)
        if noise_g is not None:
            noise_g, noise_h = check_move_noise(noise_g, noise_h, M, k_moves, B, D)
        mix = self._mixture()
        if sel is not None:
            if mix is None:
                raise _ops.FabhipError("sel (branch uniforms) belongs to a DefensiveMixtureDistribution base distribution")
            if not torch.is_tensor(sel) or sel.dtype != torch.float32 or tuple(sel.shape) != (B,):
                raise _ops.FabhipError(f"sel must be a float32 tensor of shape [{B}] (one uniform per chain)")
            sel = sel.contiguous()
        shared = (*head, eps0, noise_a, noise_b, *slots, bool(want_base), _ops.precision_of(flow))
        if mix is None and tau is None and k_moves == 0:
            out = ops.ais_run(*shared)
        else:
            # the same call with its modes named (ais_run_ext): SMC mode (resampling step in front of every transition, decided on
            # the device), the defensive mixture (16-chain tiles, fp32; composes with the SMC mode), flow-proposal moves
            if mix is not None:
                mix._refuse_fast()
            out = ops.ais_run_ext(*shared, tau, noise_r, bool(trace), RESAMPLE_METHODS[self.resample_method],
                                  *(mix.mix_args() if mix is not None else (None, None, None)), sel, mix is not None,
                                  k_moves, noise_g, noise_h)
            if tau is not None:
                self.last_smc = tuple(out[10:14])
            if k_moves > 0:
                self.last_flow_moves = out[14]
        x, lq, lp, gq, gp, log_w, n_valid, stats, base_x, base_lw = out[:10]
        point = Point(x, lq, lp, gq if hmc else None, gp if hmc else None)
        return point, log_w, n_valid, stats, base_x, base_lw

    # ---- repeated identical calls: the NEXT call's chain initialisation behind this call's device-to-host read ------------------
    # A fused call ends in a blocking 72-byte read; between that read and the next call's first kernel the GPU idles for the
    # host's post- and pre-processing (~85 us of a 4.3 ms call at the headline shape).  When a call repeats the previous one
    # unchanged (same batch, same parameter values, same operator settings: evaluation loops, the benchmark), the call runs in
    # two pieces of the SAME code (fabhip_ais_phase: INIT, then transitions 1 .. M + FINISH) and enqueues the next call's INIT
    # piece - its base noise drawn from the generator in the order the next call would draw it - right behind its own read.
    # Same kernels, same draws in the same order: results are bit-identical with the switch on or off.  The prefetched piece is
    # used only if the call it was made for arrives unchanged AND the device generator is exactly where the prefetch left it; a
    # changed key (a training step moved the parameters, another batch size, ...) drops it and rewinds the generator over its one
    # draw, so the call draws what it would have drawn; a generator the caller has touched meanwhile (set_rng_state, manual_seed,
    # any draw) drops it without a rewind.  `prefetch = False` turns the mechanism off.
    prefetch = True

    def _pf_key(self, flow, target, op, B):
        tg = tuple(id(t) if torch.is_tensor(t) else (tuple(t) if isinstance(t, (list, tuple)) else t)
                   for t in target.native_target())
        return (B, flow._packed_key, flow.__dict__.get("_pack_count", 0), tg, id(self.B_space), getattr(self.B_space, "_version", None), self.alpha,
                bool(self.p_target), _ops.precision_of(flow), op.L, op.n_outer, float(op.max_grad), float(op.target_p_accept),
                bool(op.eval_mode), id(op.mass_vector), op.mass_vector._version, int(_ops.load().get_fast_mode()))

    # ---- the fused call's arguments: ONE description, shared by every route into the ops ----------------------------------------
    @property
    def _alpha_arg(self) -> float:
        """`alpha` as the ops take it (their `float alpha` is not read when the AIS target is p)."""
        return float(self.alpha) if self.alpha is not None else 0.0

    def _call_head(self, flow, target, transition, betas=None) -> tuple:
        """The leading arguments of ais_run / ais_run_ext / ais_phase / ais_sharded_tuned: flow image, target, betas, alpha,
        p_target, transition kind.  (`betas`: a per-call list in place of B_space - the stepped adaptive driver's.)"""
        op = self.transition_operator
        if bool(op.p_target) != bool(self.p_target) or (not self.p_target and op.alpha != self.alpha):
            # the reference keeps the two in sync through FABModel.set_ais_target (core.py:102-110)
            raise _ops.FabhipError("AIS and transition operator disagree on p_target / alpha")
        return (*flow.native(), *target.native_target(), self._betas() if betas is None else betas, self._alpha_arg,
                bool(self.p_target), transition)

    def new_phase_state(self, b, eps0=None, noise_a=None, noise_b=None, draw_noise: bool = True, slab: bool = False) -> dict:
        """The caller-owned tensors of one AIS call made in pieces (`enqueue_phase`): Point fields, log_w, the 18-word
        stats[16] | n_valid[2] buffer that ONE device->host read fetches (_ops.read_counts_and_stats), the noise and, with
        `slab`, the buffer of the acceptance sums of a deferred adaptation.  Noise that is not passed in is drawn here, in the
        order the one-op call draws it (eps0, noise_a, noise_b); `draw_noise=False` only allocates noise_a / noise_b - the
        prefetch path fills them (`normal_()` / `exponential_()`: the same draws) when the call they belong to runs, so that
        the generator is consumed in call order."""
        ops = _ops.load()
        self._refuse_mixture("a call made in pieces (fabhip_ais_phase: sharded chains, the prefetch of repeated calls)")
        flow, _ = self._native_parts()
        kind, slots = operator_slots(self.transition_operator)
        hmc, b, D, M, n = kind == _ops.TRANSITION_HMC, int(b), flow.dim, self.n_intermediate_distributions, int(slots.n_inner)
        f32 = dict(dtype=torch.float32, device=flow._nf_model.q0.loc.device)
        counts_stats = torch.zeros(18, **f32)
        st = {"b": b, "cs": counts_stats, "stats": counts_stats[:16], "n_valid": counts_stats[16:18].view(torch.int32),
              "eps0": torch.randn((b, D), **f32) if eps0 is None else eps0.contiguous()}
        if not draw_noise:
            st["noise_a"], st["noise_b"] = torch.empty((M, n, b, D), **f32), torch.empty((M, n, b), **f32)
        else:
            st["noise_a"] = torch.randn((M, n, b, D), **f32) if noise_a is None else noise_a.contiguous()
            if noise_b is not None:
                st["noise_b"] = noise_b.contiguous()
            else:
                st["noise_b"] = torch.empty((M, n, b), **f32).exponential_(1.0) if hmc else torch.rand((M, n, b), **f32)
        st.update(x=torch.empty((b, D), **f32), lq=torch.empty(b, **f32), lp=torch.empty(b, **f32),
                  gq=torch.empty((b, D), **f32) if hmc else None, gp=torch.empty((b, D), **f32) if hmc else None,
                  log_w=torch.empty(b, **f32), slab=None)
        if slab:
            n_slab = ops.hmc_partials_floats(b) if hmc else ops.metropolis_partials_floats(b, M, n)
            st["slab"] = torch.empty(int(n_slab), **f32)
        return st

    def enqueue_phase(self, st, phases, j0, j1, partials=None, tune: Optional[bool] = None, logging: bool = True):
        """torch.ops.fabhip.ais_phase on a state of `new_phase_state`: the phases (FABHIP_AIS_INIT = 1, _FINISH = 2) and the
        transitions j0 .. j1 of this sampler's call.  `tune` overrides the operator's own setting (with `partials` the
        adaptation is deferred to the caller); `logging=False`: the operator's logging slots are left alone."""
        self._refuse_mixture("a call made in pieces (fabhip_ais_phase: sharded chains, the prefetch of repeated calls)")
        flow, target = self._native_parts()
        kind, s = operator_slots(self.transition_operator)
        log = s[8:] if logging else (None, None, None, None)
        _ops.load().ais_phase(*self._call_head(flow, target, kind), int(phases), int(j0), int(j1), st["eps0"], st["noise_a"],
                              st["noise_b"], *s[:7], s.tune if tune is None else bool(tune), st["x"], st["lq"], st["lp"],
                              st["gq"], st["gp"], st["log_w"], st["n_valid"], st["stats"], partials, *log, None, None,
                              _ops.precision_of(flow))

    # ---- adaptive schedule: the call stepped transition by transition, the next temperature chosen on the device ---------------
    def _run_adaptive(self, batch_size, eps0, noise_a, noise_b, want_base, noise_r, trace, force_betas, noise_g=None,
                      noise_h=None):
        """`run` with distribution_spacing_type="adaptive" (definition: tests/adaptive_spec.py).  FABHIP_AIS_INIT at beta_1 := 0,
        then per step: [resampling step +] transition j at beta_j through the phase op (betas[j] = betas[j + 1] = beta_j: no
        increment inside), fabhip_next_beta on the new point, ONE 32-byte read, the increment (fabhip_log_w_update: the fused
        kernels' expression; the first weight through fabhip_log_w_first: the chain initialisation's).  FABHIP_AIS_FINISH last.
        Once beta has reached 1 the remaining transitions run on the target without a decision or an increment.
        With n_flow_moves: fabhip::flow_move at beta_j between the resampling step and the transition of step j."""
        ops = _ops.load()
        flow, target = self._native_parts()
        kind, s = operator_slots(self.transition_operator)
        B, M = int(batch_size), self.n_intermediate_distributions
        alpha, p_target, rho, prec = self._alpha_arg, bool(self.p_target), self.ess_decay, _ops.precision_of(flow)
        tau = self.resample_threshold
        forced = None if force_betas is None else check_schedule(force_betas, M, "force_betas").tolist()
        st = self.new_phase_state(B, eps0, noise_a, noise_b)
        dev = st["x"].device
        smc = ()
        if noise_r is not None and tau is None:
            raise _ops.FabhipError("noise_r belongs to the SMC mode: set resample_threshold first")
        if tau is not None:
            noise_r = torch.rand(M, dtype=torch.float64, device=dev) if noise_r is None else check_noise_r(noise_r, M)
            rec = (torch.zeros(M, dtype=torch.int32, device=dev), torch.zeros(M, dtype=torch.float32, device=dev),
                   torch.zeros((M, B), dtype=torch.int32, device=dev) if trace else None,
                   torch.zeros((M, B), dtype=torch.float32, device=dev) if trace else None)
            smc = (tau, noise_r, False, *rec, RESAMPLE_METHODS[self.resample_method])
        base = (torch.empty_like(st["x"]), torch.empty_like(st["log_w"])) if want_base else (None, None)
        k_moves = self.n_flow_moves
        if k_moves > 0:                                                          # (drawn behind noise_a / noise_b, g before h)
            D = st["x"].shape[1]
            if noise_g is None:
                noise_g = torch.randn((M, k_moves, B, D), dtype=torch.float32, device=dev)
                noise_h = torch.empty((M, k_moves, B), dtype=torch.float32, device=dev).exponential_(1.0)
            else:
                noise_g, noise_h = check_move_noise(noise_g, noise_h, M, k_moves, B, D)
            fracs = []

        def phase(phases, j0, j1, betas, base=(None, None), part=None):
            """(`part`: "resample" / "transition" runs that half of a step alone; None: the whole step)"""
            args = (*self._call_head(flow, target, kind, betas), phases, j0, j1, st["eps0"], st["noise_a"], st["noise_b"],
                    *s[:8], st["x"], st["lq"], st["lp"], st["gq"], st["gp"], st["log_w"], st["n_valid"], st["stats"], None,
                    *s[8:], *base, prec)
            if smc and j0 <= j1 and part != "transition":
                ops.ais_phase_smc(*args, smc[0], smc[1], part == "resample", *smc[3:])
            else:
                ops.ais_phase(*args)

        def step(j, beta):
            """Step j at beta: [resampling step,] [moves,] transition."""
            if k_moves == 0:
                return phase(0, j, j, at(j, beta))
            if smc:
                phase(0, j, j, at(j, beta), part="resample")
            head = self._call_head(flow, target, kind)[:8]                       # (flow image, target)
            for m in range(k_moves):
                fracs.append(ops.flow_move(*head, st["x"], st["lq"], st["lp"], st["gq"], st["gp"], st["n_valid"], float(beta),
                                           alpha, p_target, noise_g[j - 1, m], noise_h[j - 1, m], prec)[0])
            phase(0, j, j, at(j, beta), part="transition")

        def at(j, beta):                         # the per-call betas of transition j: betas[j] = betas[j + 1] = beta
            b = [0.0] * (M + 2)
            b[j] = b[j + 1] = float(beta)
            return b

        decisions = []

        def decide(step, beta):
            out = ops.next_beta(st["log_w"], st["lq"], st["lp"], st["n_valid"], float(beta), alpha, p_target, rho, NEXT_BETA_ITERS)
            seen = (st["log_w"].clone(), st["lq"].clone(), st["lp"].clone()) if trace else None
            v = _ops._read_small(out).tolist()                                   # the step's one device->host read
            decisions.append(AdaptiveDecision(step, float(beta), v[0], v[1], v[2], int(v[3]) & 0xffff, int(v[3]) >= 65536, seen))
            return v[0]

        phase(1, 1, 0, at(0, 0.0), base)                                         # FABHIP_AIS_INIT with betas[1] = 0
        b1 = decide(0, 0.0)
        chosen = [0.0, forced[1] if forced is not None else b1]
        if chosen[1] != 0.0:
            ops.log_w_first(st["lq"], st["lp"], chosen[1], alpha, p_target, st["log_w"])
        for j in range(1, M + 1):
            bj = chosen[j]
            step(j, bj)
            nxt = 1.0
            if j < M:
                nxt = decide(j, bj) if bj < 1.0 else 1.0
                if forced is not None:
                    nxt = forced[j + 1]
            if nxt != bj:
                ops.log_w_update(st["lq"], st["lp"], bj, nxt, alpha, p_target, st["log_w"])
            chosen.append(nxt)
        phase(2, 1, 0, at(M, chosen[M]))                                         # FABHIP_AIS_FINISH
        self.last_betas = torch.tensor(chosen, dtype=torch.float64)
        self.last_adaptive = decisions
        self.__dict__["_adaptive_info"] = {
            "beta_1": float(chosen[1]), "n_steps_to_beta_one": int(next(i for i, b in enumerate(chosen) if b >= 1.0)),
            "n_bisect_floor": int(sum(d.floor for d in decisions))}
        if k_moves > 0:
            self.last_flow_moves = torch.cat(fracs).view(M, k_moves)
        if tau is not None:
            empty = torch.empty(0, device=dev)
            self.last_smc = (rec[0], rec[1], rec[2] if trace else empty.int(), rec[3] if trace else empty)
        hmc = kind == _ops.TRANSITION_HMC
        point = Point(st["x"], st["lq"], st["lp"], st["gq"] if hmc else None, st["gp"] if hmc else None)
        return point, st["log_w"], st["n_valid"], st["stats"], base[0], base[1]

    def _pf_take(self, key):
        """The prefetched piece made for `key`, if the generator is where the prefetch left it; else it is dropped (and, when only
        the key changed, the generator rewound over the prefetch's draw)."""
        pf = self.__dict__.pop("_pf_state", None)
        if pf is None:
            return None
        k, st, before, after, dev = pf
        untouched = torch.equal(torch.cuda.get_rng_state(dev), after)
        if untouched and k == key:
            return st
        if untouched:
            torch.cuda.set_rng_state(before, dev)
        return None

    def _sample_repeated(self, B, key):
        """One call in two pieces with the next call's chain initialisation enqueued behind this call's read (see above)."""
        M = self.n_intermediate_distributions
        st = self._pf_take(key)
        if st is None:
            st = self.new_phase_state(B, draw_noise=False)
            self.enqueue_phase(st, 1, 1, 0)                                      # FABHIP_AIS_INIT (reads eps0 only)
        st["noise_a"].normal_()
        st["noise_b"].exponential_(1.0)
        self.enqueue_phase(st, 2, 1, M)                                          # transitions 1 .. M, FABHIP_AIS_FINISH

        dev = st["x"].device

        def enqueue_next():
            before = torch.cuda.get_rng_state(dev)
            nxt = self.new_phase_state(B, draw_noise=False)
            after = torch.cuda.get_rng_state(dev)
            self.enqueue_phase(nxt, 1, 1, 0)
            self.__dict__["_pf_state"] = (key, nxt, before, after, dev)
        host, counts = _ops.read_counts_and_stats(st["n_valid"], st["stats"], between=enqueue_next)
        return Point(st["x"], st["lq"], st["lp"], st["gq"], st["gp"]), st["log_w"], host, counts

    def _betas(self):
        """B_space as a list of Python floats (the ops' `float[] betas`), converted once per B_space tensor / version."""
        bs = self.B_space
        c = self.__dict__.get("_betas_cache")
        ver = getattr(bs, "_version", None)
        if c is None or c[0] is not bs or c[1] != ver:
            c = (bs, ver, [float(b) for b in bs])
            self.__dict__["_betas_cache"] = c
        return c[2]

    def perform_transition(self, x_new: Point, log_w: torch.Tensor, j: int):
        """ais.py:90-105: one MCMC transition towards the j-th intermediate distribution + the log-weight increment
        (skipped when beta does not change).  The fused call does the same for all j inside `fabhip_ais_run`.
        One LOCAL transition: `n_flow_moves` does not act here (the flow-proposal moves belong to the whole call)."""
        self._refuse_adaptive("perform_transition (one transition of a FIXED schedule)",
                              "run the whole call (sample_and_log_weights / run), or give the sampler a schedule of your own")
        beta, beta_next = float(self.B_space[j]), float(self.B_space[j + 1])
        log_w = log_w.detach().clone().contiguous()
        x_new = self.transition_operator.transition(x_new, j, beta, log_w=log_w if beta_next != beta else None,
                                                    beta_next=beta_next)
        return x_new, log_w

    @property
    def is_native(self) -> bool:
        if self._mixture() is not None:
            # the fused call evaluates the mixture itself; the operator (whose own `is_native` speaks of a plain RealNVP: stepped
            # from Python it evaluates the mixture through the plug-in) only has to be this package's, over the same plug-ins
            op = self.transition_operator
            return _owner_or_none(self.target_log_prob, _NativeTarget) is not None and \
                isinstance(op, (HamiltonianMonteCarlo, Metropolis)) and \
                _owner_or_none(op.base_log_prob, DefensiveMixtureDistribution) is self.base_distribution and \
                _owner_or_none(op.target_log_prob, _NativeTarget) is not None
        return isinstance(self.base_distribution, RealNVP) and \
            _owner_or_none(self.target_log_prob, _NativeTarget) is not None and self.transition_operator.is_native

    def _resample_generic(self, point: Point, log_w: torch.Tensor, u: torch.Tensor, record: list):
        """The resampling step of the generic path: the decision op (fabhip::smc_decide - the fused call's own kernel) + the
        existing row gather; no host synchronisation (the gather runs with identity ancestors when nothing is resampled)."""
        ops = _ops.load()
        log_w = log_w.contiguous()
        anc, flag, ess, common = ops.smc_decide(log_w, float(self.resample_threshold), u, RESAMPLE_METHODS[self.resample_method])
        g = lambda t: None if t is None else ops.gather_rows(t.detach().contiguous().float().view(t.shape[0], -1),      # noqa: E731
                                                             anc).view(t.shape)
        point = Point(g(point.x), g(point.log_q), g(point.log_p), g(point.grad_log_q), g(point.grad_log_p))
        record.append((flag, ess, anc, log_w))
        return point, torch.where(flag.bool(), common, log_w)

    def _sample_generic(self, batch_size: int, logging: bool, noise_a=None, noise_b=None, want_base: bool = False,
                        raise_at_end: bool = True, noise_r=None):
        """ais.py:53-105 for ANY `Distribution` / `LogProbFunc` plug-ins (fab/types_.py:5-27): the reference's loop,
        stepped from Python; the plug-ins evaluate their own densities, the transitions / log-weight arithmetic /
        ESS run as fabhip kernels (transition_operators.py: generic path).  Explicit noise (parity replays): after the
        chain-init filter has dropped rows, noise row i belongs to the i-th SURVIVING chain - the reference draws
        `randn_like(point.x)` of the filtered shape (hmc.py:134), and the fused path indexes its noise the same way."""
        ops = _ops.load()
        op = self.transition_operator
        B, M = int(batch_size), self.n_intermediate_distributions
        alpha = self._alpha_arg
        x, log_q0 = self.base_distribution.sample_and_log_prob((B,))
        point = create_point_generic(x, self.base_distribution.log_prob, self.target_log_prob,
                                     with_grad=op.uses_grad_info, log_q_x=log_q0)
        log_q0 = log_q0.detach().contiguous().float()
        log_w = ops.anneal_log_prob(point.log_q, point.log_p, float(self.B_space[1]), alpha, bool(self.p_target)) - log_q0
        base = None
        if want_base:                                      # generate_eval_data (ais.py:152-166): log p - log q of the sampling pass
            valid = torch.isfinite(point.log_p) & torch.isfinite(point.log_q)
            base = (point.x[valid].clone(), (point.log_p - log_q0)[valid])
        point, log_w = self._remove_nan_and_infs(point, log_w, "chain init")
        ess_base = ops.ess_logz((point.log_p - point.log_q).contiguous(), None, 1.0)
        hmc = isinstance(op, HamiltonianMonteCarlo)
        n_inner = op.n_outer if hmc else op.n_updates
        smc_on, record = self.resample_threshold is not None, []
        if smc_on:                                          # (drawn after the plug-ins' own draws of the chain initialisation)
            noise_r = (torch.rand(M, dtype=torch.float64, device=log_w.device) if noise_r is None
                       else check_noise_r(noise_r, M).to(log_w.device))
        for j in range(1, M + 1):
            if smc_on:
                point, log_w = self._resample_generic(point, log_w, noise_r[j - 1:j], record)
            n = point.x.shape[0]
            beta, beta_next = float(self.B_space[j]), float(self.B_space[j + 1])
            lw = log_w if beta_next != beta else None                              # ais.py:93
            na = noise_a[j - 1][:, :n].contiguous() if noise_a is not None else None
            nb = noise_b[j - 1][:, :n].contiguous() if noise_b is not None else None
            if hmc:
                point = op.transition(point, j, beta, log_w=lw, beta_next=beta_next, noise_p=na, noise_e=nb)
            else:
                point = op.transition(point, j, beta, log_w=lw, beta_next=beta_next, noise_x=na, noise_u=nb)
        point, log_w = self._remove_nan_and_infs(point, log_w, "chain end", raise_exception=raise_at_end)
        if smc_on:
            self.last_smc = (torch.cat([r[0] for r in record]), torch.cat([r[1] for r in record]),
                             torch.stack([r[2] for r in record]).int(), torch.stack([r[3] for r in record]))
        if logging:
            st = torch.cat([ess_base[:1], ops.ess_logz(log_w.contiguous(), None, float(B))[:2]]).tolist()
            self._logging_info = LoggingInfo(ess_base=st[0], ess_ais=st[1], log_Z=st[2])
            self._log_smc()
        if want_base:
            return point, log_w.detach(), base
        return point, log_w.detach()

    @staticmethod
    def _remove_nan_and_infs(point: Point, log_w: torch.Tensor, descriptor: str, raise_exception: bool = True):
        """ais.py:190-213 (generic path; the fused path compacts on the device)."""
        valid = torch.isfinite(point.log_p) & torch.isfinite(point.log_q)
        n_valid = int(valid.sum())
        if n_valid == 0:
            if raise_exception:
                raise NoValidPoints(descriptor.replace("chain ", ""))
            print(f"No valid points generated in sampling the {descriptor}")       # ais.py:206-207 (evaluation)
            return point, log_w
        if n_valid == valid.shape[0]:
            return point, log_w
        print(f"{valid.shape[0] - n_valid} nan/inf samples/log-probs/log-weights encountered at {descriptor}.")
        keep = valid.nonzero().flatten()
        g = lambda t: None if t is None else t[keep].contiguous()      # noqa: E731
        return Point(g(point.x), g(point.log_q), g(point.log_p), g(point.grad_log_q), g(point.grad_log_p)), g(log_w)

    def _log_smc(self):
        """n_resampled / ess_min_in_chain of the call that just ended (SMC mode only): one more small read, after the call's own."""
        self.__dict__["_smc_info"] = None
        if self.resample_threshold is not None and self.last_smc is not None:
            flag, ess = self.last_smc[0], self.last_smc[1]
            h = torch.stack([flag.float().sum(), ess.min()]).tolist()
            self.__dict__["_smc_info"] = {"n_resampled": int(h[0]), "ess_min_in_chain": float(h[1])}

    def _log_flow_moves(self):
        """flow_move_p_accept_dist0 / dist{M-1} of the call that just ended (moves on only): means over the k moves of the
        first / last step; one more small read, after the call's own."""
        self.__dict__["_flow_move_info"] = None
        fm = self.last_flow_moves
        if self.n_flow_moves > 0 and fm is not None and fm.numel() > 0:
            M = fm.shape[0]
            h = torch.stack([fm[0].mean(), fm[M - 1].mean()]).tolist()
            self.__dict__["_flow_move_info"] = {"flow_move_p_accept_dist0": float(h[0]),
                                                f"flow_move_p_accept_dist{M - 1}": float(h[1])}

    def sample_and_log_weights(self, batch_size: int, logging: bool = True, eps0=None, noise_a=None, noise_b=None,
                               u0=None, noise_r=None, sel=None, noise_g=None, noise_h=None) -> Tuple[Point, torch.Tensor]:
        self._refuse_adaptive_routes()
        self._refuse_flow_move_routes()
        fused_spline = self._spline_parts() is not None
        # (SMC mode, adaptive schedules, flow-proposal moves: all step outside the plain phase op's pieces)
        smc_on = self.resample_threshold is not None or self.adaptive or self.n_flow_moves > 0
        mix_on = self._mixture() is not None and self.is_native
        if sel is not None and not mix_on:
            raise _ops.FabhipError("sel (branch uniforms) belongs to the fused call over a DefensiveMixtureDistribution base")
        if fused_spline:
            self._refuse_resampling("the fused spline-flow call")
        if noise_r is not None and self.resample_threshold is None:
            raise _ops.FabhipError("noise_r belongs to the SMC mode: set resample_threshold first")
        if u0 is not None and not fused_spline:               # (it used to be dropped silently)
            raise _ops.FabhipError("u0 (uniform base draws) belongs to the fused spline-flow call: this sampler's base "
                                   "distribution / transition operator does not take that path")
        if not self.is_native and not fused_spline:
            if eps0 is not None:
                raise _ops.FabhipError("eps0 is the base noise of a fab_torch_amd RealNVP; a generic base_distribution "
                                       "draws its own samples in sample_and_log_prob")
            return self._sample_generic(batch_size, logging, noise_a, noise_b, noise_r=noise_r)
        repeated = None
        # (SMC mode, defensive mixture: the prefetch of repeated calls is bypassed - its pieces run through the plain phase op)
        if (not fused_spline and not smc_on and not mix_on and self.prefetch and eps0 is None and noise_a is None and noise_b is None
                and isinstance(self.transition_operator, HamiltonianMonteCarlo)):
            flow, target = self._native_parts()
            flow.native()                                                        # (the image - and its key - of the current parameters)
            key = self._pf_key(flow, target, self.transition_operator, int(batch_size))
            if self.__dict__.get("_pf_last_key") == key:
                repeated = self._sample_repeated(int(batch_size), key)
            else:
                self._pf_take(None)                                              # (drops a piece made for another key)
            self.__dict__["_pf_last_key"] = key
        if repeated is not None:
            point, log_w, host, (n_init, n_end) = repeated
        else:
            if fused_spline:
                point, log_w, n_valid, stats, _, _ = self._run_spline(batch_size, eps0, noise_a, noise_b, u0=u0)
            else:
                if smc_on:
                    self._pf_take(None)                                          # (a piece prefetched before the mode was set)
                    self.__dict__.pop("_pf_last_key", None)
                point, log_w, n_valid, stats, _, _ = self.run(batch_size, eps0, noise_a, noise_b, noise_r=noise_r, sel=sel,
                                                              noise_g=noise_g, noise_h=noise_h)
            host, (n_init, n_end) = _ops.read_counts_and_stats(n_valid, stats)   # the single device->host read
        if n_init == 0:
            raise NoValidPoints("init")
        if n_end == 0:
            raise NoValidPoints("end")
        if n_end != batch_size:
            print(f"{batch_size - n_end} nan/inf samples/log-probs/log-weights encountered.")
            point, log_w = point[:n_end], log_w[:n_end]
        st = host
        if logging:
            self._logging_info = LoggingInfo(ess_base=float(st[0]), ess_ais=float(st[3]), log_Z=float(st[4]))
            self._log_smc()
            self._log_flow_moves()
        return point, log_w.detach()

    def generate_eval_data(self, outer_batch_size: int, inner_batch_size: int):
        """ais.py:132-188 — evaluation batches: the chains' starting points (flow samples) with log p - log q, and
        the AIS samples with their log-weights.  Everything stays on the device: the batches are enqueued back to
        back and the row counts of all of them are read with ONE device->host copy at the end (the reference
        concatenates on the CPU after a `.cpu()` per batch); the returned tensors live on the GPU.  Generic plug-ins
        (e.g. the spline flow): the reference's loop per batch through `_sample_generic`."""
        assert outer_batch_size % inner_batch_size == 0
        self._refuse_adaptive_routes()
        n_batches = outer_batch_size // inner_batch_size
        B = inner_batch_size
        if not self.is_native and self._spline_parts() is None:
            bx, blw, ax, alw = [], [], [], []
            for _ in range(n_batches):
                point, log_w, base = self._sample_generic(B, logging=False, want_base=True, raise_at_end=False)
                bx.append(base[0]); blw.append(base[1]); ax.append(point.x.detach()); alw.append(log_w)
            return torch.cat(bx), torch.cat(blw), torch.cat(ax), torch.cat(alw)
        base_x, base_lw, ais_x, ais_lw, counts = [], [], [], [], []
        for i in range(n_batches):
            point, log_w, n_valid, _, bx, blw = self.run(B, want_base=True)
            base_x.append(bx)
            base_lw.append(blw)
            ais_x.append(point.x)
            ais_lw.append(log_w)
            counts.append(n_valid)
        host = torch.stack(counts).cpu()                       # the single synchronisation
        if int(host[:, 0].min()) == 0:
            raise NoValidPoints("init")
        n0 = [int(v) for v in host[:, 0]]
        n1 = [int(v) if int(v) > 0 else n0[i] for i, v in enumerate(host[:, 1])]   # "chain end": print + keep (:170)
        if any(int(v) == 0 for v in host[:, 1]):
            print("No valid points generated in sampling the chain end")
        return (torch.cat([base_x[i][:n0[i]] for i in range(n_batches)]),
                torch.cat([base_lw[i][:n0[i]] for i in range(n_batches)]),
                torch.cat([ais_x[i][:n1[i]] for i in range(n_batches)]),
                torch.cat([ais_lw[i][:n1[i]] for i in range(n_batches)]))
