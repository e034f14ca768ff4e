"""Records tests/golden/g20_r4f_nsplit.npz: what a tuned and a frozen-step-size fused AIS call on seeded noise return at 4-chain
tiles for the cases of tests/test_gpu_r4f_nsplit.py (x, log_w, log_q, grad_log_q, step sizes), fast mode included.  Run on the
commit whose bits are to be kept - the fixture in the tree was recorded with the K-split stages, the parent of the N-split
hidden-width products - on the GPU:
    python tools/record_r4f_nsplit.py [output.npz]
The cases, flows and noise are the test module's own functions, so the test replays exactly what was recorded."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.set_num_threads(1)                 # (what tests/conftest.py gives a GPU test)

import test_gpu_r4f_nsplit as t         # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", t.FIXTURE)
rec = {}
for D, nodes in t.SHAPES:
    rec[f"probe_D{D}_n{nodes}"] = t.weight_probe(D, nodes)
for fast, cases in ((False, t.CASES), (True, t.FAST_CASES)):
    for D, nodes, B, ev in cases:
        key = t.case_key(D, nodes, B, ev, fast=fast)
        a, b = t.ais_call(D, nodes, B, eval_mode=ev, fast=fast), t.ais_call(D, nodes, B, eval_mode=ev, fast=fast)
        for name in t.RECORDED:
            assert torch.equal(a[name], b[name]), f"{key}: {name} is not reproducible"
            rec[f"{key}.{name}"] = a[name].numpy()
        print(key, "log_w", a["log_w"].numpy(), "epsilons", a["epsilons"].numpy().ravel())
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
np.savez_compressed(out, **rec)
print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(rec)} arrays")
