"""Shared helpers for the test-suite (fixtures loading, tolerances)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

# BASELINE.json north_star: "log-weights and flow log-probs within 1e-4 relative fp32"
RTOL = 1e-4


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def close(a, b, rtol=RTOL, atol=None, atol_scale=1.0):
    """Element-wise |a-b| <= atol + rtol*|b| (numpy.isclose form) with rtol = 1e-4 (north_star) and a SMALL absolute
    floor for entries near zero: atol = 2e-6 * max(1, max|b|) by default, i.e. ~16 fp32 ulps of the largest entry
    (entries of one tensor are sums of terms of that magnitude, so a cancelling entry cannot be more accurate than
    that in fp32 whatever the summation order) — 50x tighter than the former "1e-4 of the largest entry".
    Non-finite patterns must agree exactly."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    if a.shape != b.shape:
        return False
    if not np.array_equal(np.isfinite(a), np.isfinite(b)):
        return False
    fin = np.isfinite(b)
    if not fin.any():
        return True
    a64, b64 = a[fin].astype(np.float64), b[fin].astype(np.float64)
    if atol is None:
        atol = 2e-6 * max(1.0, float(np.abs(b64).max())) * atol_scale
    return bool(np.all(np.abs(a64 - b64) <= atol + rtol * np.abs(b64)))


def worst(a, b, rtol=RTOL):
    """(max |a-b| / (atol + rtol |b|)) diagnostic for assertion messages: <= 1 passes `close`."""
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    fin = np.isfinite(b)
    if not fin.any():
        return 0.0
    a64, b64 = a[fin].astype(np.float64), b[fin].astype(np.float64)
    atol = 2e-6 * max(1.0, float(np.abs(b64).max()))
    return float(np.max(np.abs(a64 - b64) / (atol + rtol * np.abs(b64))))


def max_rel_err(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    fin = np.isfinite(b)
    scale = max(1.0, float(np.abs(b[fin]).max())) if fin.any() else 1.0
    return float(np.abs(a[fin].astype(np.float64) - b[fin].astype(np.float64)).max()) / scale if fin.any() else 0.0


def oracle_flow_from_golden(g):
    """Rebuild the oracle RealNVP whose state_dict is stored in a fixture under 'flow.*'."""
    from oracle import flow as oflow
    sd = {k[len("flow."):]: torch.tensor(v) for k, v in g.items() if k.startswith("flow.")}
    D = sd["q0.loc"].shape[1]
    K = len([k for k in sd if k.endswith(".log_S")])
    W = sd["flows.0.flows.1.param_map.net.0.weight"].shape[0]
    assert W % D == 0
    nf = oflow.make_realnvp(D, K, W // D)
    nf.load_state_dict(sd)
    return nf


def seeded_oracle_flow(dim, n_layers, nodes, seed, std=0.05):
    """The oracle RealNVP with seeded parameters: torch.manual_seed(seed) -> nn.Linear default initialisation and the
    QR-based InvertibleAffine of oracle.flow.make_realnvp, last coupling Linear re-drawn N(0, std^2) with seed + 1 (the
    reference's `init_zeros` makes an untrained flow the identity).  tests/golden/make_golden.py builds the flow of the
    g14 fixtures with this very function, so the fixtures store the seed instead of 4.8 MB of weights."""
    from oracle import flow as oflow
    torch.manual_seed(seed)
    nf = oflow.make_realnvp(dim, n_layers, nodes)
    oflow.randomize_last_layers(nf, std=std, seed=seed + 1)
    return nf


def flow_from_g14(g):
    """The oracle flow of a g14 fixture, rebuilt from its seed and checked against the stored weight probe."""
    nf = seeded_oracle_flow(int(g["D"]), int(g["K"]), int(g["nodes"]), int(g["flow_seed"]), float(g["flow_std"]))
    probe = torch.stack([nf.flows[0].flows[1].param_map.net[2].weight[0, :8].detach(),
                         nf.flows[-2].flows[1].param_map.net[4].weight[1, :8].detach()])
    assert np.array_equal(probe.numpy(), g["flow_probe"]), "seeded flow differs from the one the fixture was made with"
    return nf


def param_probes(tensors, seed, n=16):
    """A probe of every tensor of a parameter list, [len(tensors), n + 2] float64: n entries at seeded positions (one generator for
    the whole list, drawn in order), the tensor's sum and its squared norm.  The g18 fixtures store these instead of 4.8 MB of
    parameters per snapshot (tests/golden/make_golden.py)."""
    g = torch.Generator().manual_seed(int(seed))
    out = []
    for t in tensors:
        flat = t.detach().reshape(-1).cpu().double()
        pos = torch.randint(flat.numel(), (n,), generator=g)
        out.append(torch.cat([flat[pos], flat.sum().reshape(1), (flat * flat).sum().reshape(1)]).numpy())
    return np.stack(out)


def probes_close(params, seed, ref, rtol):
    """`param_probes(params, seed)` against a stored probe: the sampled entries of every tensor at `close(rtol)` (floor from that
    tensor's own probe), its sum and squared norm at rtol relative to the sum of absolute entries / the squared norm.
    Returns the list of (tensor index, what) that miss."""
    got, bad = param_probes(params, seed), []
    for i, (a, b, t) in enumerate(zip(got, ref, params)):
        if not close(a[:-2], b[:-2], rtol):
            bad.append((i, "entries", worst(a[:-2], b[:-2], rtol)))
        l1 = float(t.detach().abs().double().sum())
        if abs(a[-2] - b[-2]) > rtol * max(l1, 1e-30) or abs(a[-1] - b[-1]) > 2 * rtol * max(abs(b[-1]), 1e-30):
            bad.append((i, "sums", float(a[-2] - b[-2]), float(a[-1] - b[-1])))
    return bad


def g18_oracle_replay(g, check=None, dtype=torch.float32):
    """oracle/train.py driven over a g18 trace (tests/golden/make_golden.py:g18_trainer_traces_wide) on its captured noise, from the
    seeded flow.  Returns dict(nf, hmc, buffer, starts, outs): `starts[it]` is the complete state at the start of iteration it
    (parameters, Adam moments / step, HMC step sizes, buffer contents and ring position, the carried grad_norm) - what the
    teacher-forced GPU test restarts from; `outs[it]` what oracle.train.train_iteration returned plus the buffer after it.
    `check(it, state)`: called at every iteration start and once at the end (it = n_iter) - the CPU test compares there.
    `dtype=torch.float64`: the same replay in double precision (flow, step sizes, buffer, noise cast up) - the generator's measure
    of the trace's own rounding."""
    from oracle import ais as oais, targets as otgt, train as otrain
    D, K, nodes, M, L, B = (int(g[k]) for k in ("D", "K", "nodes", "M", "L", "B"))
    alpha, n_iter, n_batches, n_init = float(g["alpha"]), int(g["n_iter"]), int(g["n_batches"]), int(g["n_init_calls"])
    nf = flow_from_g14(g).to(dtype)
    target = otgt.ManyWell(D)
    hmc = oais.HMC(M, D, nf.log_prob, target.log_prob, alpha=alpha, p_target=False, epsilon=float(g["eps_init"]), L=L, dtype=dtype)
    assert dtype != torch.float32 or np.array_equal(hmc.epsilons.numpy(), g["in_epsilons"])
    ais = oais.AIS(lambda e: tuple(t.detach() for t in nf.sample_eps(e)), nf.log_prob, target.log_prob, hmc, False, alpha, M)
    buf = otrain.Buffer(D, int(g["buf_len"]), int(g["buf_min"]), dtype=dtype)

    def T(a):
        t = torch.tensor(a)
        return t.to(dtype) if t.dtype.is_floating_point else t
    init_log_w = []
    for c in range(n_init):
        pt, lw, _ = ais.sample_and_log_weights(T(g[f"call{c}_eps0"]), T(g[f"call{c}_noise_p"]), T(g[f"call{c}_noise_e"]))
        init_log_w.append(lw.detach().clone())
        buf.add(pt.x.detach(), lw.detach(), pt.log_q.detach())
    assert buf.can_sample
    params = list(nf.parameters())
    opt = torch.optim.Adam(params, lr=float(g["lr"]))

    def state(grad_norm):
        adam = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), float(opt.state[p]["step"]))
                for p in params] if len(opt.state) else None
        return dict(params={k: v.detach().clone() for k, v in nf.state_dict().items()}, adam=adam, eps=hmc.epsilons.clone(),
                    ceps=hmc.common_epsilon.clone(), buf_x=buf.x.clone(), buf_log_w=buf.log_w.clone(),
                    buf_log_q_old=buf.log_q_old.clone(), buf_index=buf.current_index, buf_full=buf.is_full, grad_norm=grad_norm)
    starts, outs, carry = [], [], None
    for it in range(n_iter):
        starts.append(state(carry))
        if check:
            check(it, starts[-1])
        c = n_init + it
        noise = dict(eps0=T(g[f"call{c}_eps0"]), noise_p=T(g[f"call{c}_noise_p"]), noise_e=T(g[f"call{c}_noise_e"]),
                     gumbel=T(g[f"it{it}_gumbel"]), perm=T(g[f"it{it}_perm"]))
        out = otrain.train_iteration(ais, nf.log_prob, params, opt, buf, alpha, B, n_batches, noise, float(g["max_gradient_norm"]),
                                     float(g["w_adjust_max_clip"]), grad_norm=carry)
        carry = out["grad_norm_carry"]
        out["buf_log_w"], out["buf_log_q_old"] = buf.log_w.clone(), buf.log_q_old.clone()
        outs.append(out)
    final = state(carry)
    if check:
        check(n_iter, final)
    return dict(nf=nf, hmc=hmc, buffer=buf, starts=starts, outs=outs, final=final, init_log_w=init_log_w, params=params)
