"""Records tests/golden/g19_r4f_handover.npz: what one tuned AIS call on seeded noise returns at 4-chain tiles for the shapes of
tests/test_gpu_r4f_handover.py (x, log_w, log_q, step sizes).  Run on the commit whose bits are to be kept - the fixture in the
tree was recorded with the two-barrier stages, the parent of the in-wave hand-over - on the GPU:
    python tools/record_r4f_handover.py [output.npz]
The cases, flows and noise are the test module's own functions, so the test replays exactly what was recorded."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
torch.set_num_threads(1)                 # (what tests/conftest.py gives a GPU test)

import test_gpu_r4f_handover as t       # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", t.FIXTURE)
rec = {}
for D, nodes in t.SHAPES:
    rec[f"probe_D{D}_n{nodes}"] = t.weight_probe(D, nodes)
for D, nodes, B in t.CASES:
    a, b = t.ais_call(D, nodes, B), t.ais_call(D, nodes, B)
    for name in t.RECORDED:
        assert torch.equal(a[name], b[name]), f"{t.case_key(D, nodes, B)}: {name} is not reproducible"
        rec[f"{t.case_key(D, nodes, B)}.{name}"] = a[name].numpy()
    print(t.case_key(D, nodes, B), "log_w", a["log_w"].numpy(), "epsilons", a["epsilons"].numpy().ravel())
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
np.savez_compressed(out, **rec)
print(f"wrote {out}: {os.path.getsize(out)} bytes, {len(rec)} arrays")
