#!/bin/bash
# first GPU run of the fused 8-chain stages: tests that touch the 8-chain kernels, then the bench line (chains_2048)
cd "$(dirname "$0")/../.."; O=${1:?usage: bash tools/experiments/r8f_run1.sh OUT_DIR}; mkdir -p "$O"
timeout 900 python -m pytest tests/test_gpu_hmc_shapes.py -x -q -m gpu -k "eight or small_tiles or one_launch_tail" > $O/pytest1.txt 2>&1; tail -5 $O/pytest1.txt
timeout 900 python -m pytest tests/test_gpu_parity.py -x -q -m gpu -k "headline_architecture or g14 or g15" > $O/pytest2.txt 2>&1; tail -5 $O/pytest2.txt
timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err; python - "$O/bench.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['roofline']['frac'], d['roofline']['chains_2048'], d['roofline']['full_chip'])
PY
FABHIP_R4_STREAM=1 timeout 600 python bench.py --full > $O/bench_unfused.json 2>> $O/bench.err; python - "$O/bench_unfused.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['roofline']['frac'], d['roofline']['chains_2048'])
PY
