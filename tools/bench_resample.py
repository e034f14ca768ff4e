"""Resamplers side by side in ONE process, alternating: HIP-event times through the custom ops, log_w ~ 3 N(0, 1) seed 0 (what
bench.py: resample_rooflines uses), N = n_samples.  Per size and method: median and min..max of the calls, algorithmic bytes,
GB/s and the share of the HBM peak.

    python tools/bench_resample.py [--sizes 2048,16384,512000,1048576,16777216,67108864] [--calls 24] [--rounds 3] [--out FILE]
                                   [--scale 3.0] [--heavy]

`--scale S`: log_w ~ S N(0, 1); `--heavy`: two weights far above the rest (e^40 and e^38.5: giant runs, grid-wide fill).

Methods: multinomial_with_rand (torch.rand(float64) + fabhip_resample_multinomial, what `resample()` does by default),
multinomial (uniforms given), systematic, stratified, stratified_shuffled (fabhip_resample_stratified), stream_sorted,
stream_shuffled (fabhip_resample_multinomial_stream).
`--only METHOD --calls K` runs one method alone (for a kernel trace of its own)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fab_torch_amd import _ops  # noqa: E402

PEAK_HBM_TBPS = 8.0            # MI355X HBM3E spec (bench.py uses the same figure)


def times(fn, n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,16384,512000,1048576,16777216,67108864")
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, help="one method, or several separated by commas")
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--heavy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ops = _ops.load()
    dev = "cuda"
    rows = []
    for N in [int(s) for s in a.sizes.split(",")]:
        g = torch.Generator(device=dev).manual_seed(0)
        lw = torch.randn(N, device=dev, generator=g) * a.scale
        if a.heavy:
            lw[N // 6] = 40.0; lw[(5 * N) // 6] = 38.5
        u = torch.rand(N, device=dev, generator=g, dtype=torch.float64)
        methods = {
            # algorithmic bytes: log_w in, indices out (+ the uniforms in, + the uniforms written and read back)
            "multinomial_with_rand": (lambda: ops.resample_multinomial(lw, torch.rand(N, dtype=torch.float64, device=dev)), 28 * N),
            "multinomial": (lambda: ops.resample_multinomial(lw, u), 20 * N),
            "systematic": (lambda: ops.resample_systematic(lw, 0.3, N), 12 * N),
            "stratified": (lambda: ops.resample_stratified(lw, 12345, N, 0), 12 * N),
            "stratified_shuffled": (lambda: ops.resample_stratified(lw, 12345, N, 1), 12 * N),
            "stream_sorted": (lambda: ops.resample_multinomial_stream(lw, 12345, N, 0), 12 * N),
            "stream_shuffled": (lambda: ops.resample_multinomial_stream(lw, 12345, N, 1), 12 * N),
        }
        if a.only:
            methods = {k: methods[k] for k in a.only.split(",")}
        per = max(1, a.calls // a.rounds)
        for fn, _ in methods.values():              # warm-up: scratch of every method allocated, clocks up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in methods}
        for _ in range(a.rounds):                   # alternate: every method sees the same clocks / thermal state
            for k, (fn, _) in methods.items():
                t[k] += times(fn, per)
        for k, (_, alg) in methods.items():
            s = sorted(t[k])
            med = s[len(s) // 2]
            rows.append({"N": N, "scale": a.scale, "heavy": a.heavy, "method": k, "calls": len(s), "median_us": med * 1e6, "min_us": s[0] * 1e6, "max_us": s[-1] * 1e6,
                         "algorithmic_bytes": alg, "GBps": alg / med / 1e9, "frac_hbm_peak": alg / med / 1e12 / PEAK_HBM_TBPS})
            print(json.dumps(rows[-1]), flush=True)
        del lw, u, methods
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
