"""Generate tests/golden/g19_defensive_mixture.npz by RUNNING THE IMPORTED REFERENCE class
fab.trainable_distributions.defensive_mixture.DefensiveMixtureDistribution (build container only, like make_golden.py:
the reference is imported from /root/reference with its absent third-party modules stubbed).

The oracle RealNVP (oracle/flow.py, float64) is wrapped as the reference's `flow` plug-in; the fixture holds the flow's
state, the mixture parameters, x at the radii of the three regimes (flow-dominated, mixed, flow density negligible) and the
reference's `log_prob(x)`.  Only DATA is written: one small .npz of arrays.

Usage:  python tests/golden/make_golden_defensive.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

for name in ["wandb", "normflows", "nflows", "nflows.flows"]:
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["normflows"].NormalizingFlow = object
sys.modules["nflows"].flows = sys.modules["nflows.flows"]
sys.modules["nflows.flows"].Flow = object
sys.path.insert(0, os.environ.get("FAB_REFERENCE", "/root/reference"))

from fab.trainable_distributions.defensive_mixture import DefensiveMixtureDistribution  # noqa: E402

from oracle import flow as oflow  # noqa: E402

D, K, NODES, STD, SEED = 6, 2, 5, 0.3, 7
RADII = (0.5, 2.0, 4.0, 40.0, 200.0)
ROWS_PER_RADIUS = 6


def main():
    torch.manual_seed(SEED)
    nf = oflow.make_realnvp(D, K, NODES)
    oflow.randomize_last_layers(nf, std=STD, seed=SEED)
    nf = nf.double()
    ref = DefensiveMixtureDistribution(oflow.WrappedFlow(nf))
    g = torch.Generator().manual_seed(19)
    loc = torch.full((D,), 0.25, dtype=torch.float64) + 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    log_scale = torch.full((D,), 1.0, dtype=torch.float64) + 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    ref.loc = torch.nn.Parameter(loc)
    ref.log_scale = torch.nn.Parameter(log_scale)
    ref.mixture_logit = torch.nn.Parameter(torch.tensor(1.0, dtype=torch.float64))
    u = torch.randn(len(RADII) * ROWS_PER_RADIUS, D, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=1, keepdim=True)
    x = u * torch.tensor(RADII, dtype=torch.float64).repeat_interleave(ROWS_PER_RADIUS)[:, None]
    with torch.no_grad():
        lq = ref.log_prob(x)
        lq_flow = nf.log_prob(x)
    assert torch.isfinite(lq).all()
    out = {"flow." + k: v.detach().numpy() for k, v in nf.state_dict().items()}
    out.update(x=x.numpy(), loc=loc.numpy(), log_scale=log_scale.numpy(), mixture_logit=np.float64(1.0),
               log_prob=lq.numpy(), log_q_flow=lq_flow.numpy(), radii=np.asarray(RADII))
    path = os.path.join(HERE, "g19_defensive_mixture.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {os.path.basename(path)}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
