#!/bin/bash
# first GPU run of the LDS stash (FABHIP_OPT_R4_STREAM = 3): bit-identity against option 2, stage stamps, bench both ways
cd "$(dirname "$0")/../.."; O=${1:?usage: bash tools/experiments/stash_run1.sh OUT_DIR}; mkdir -p "$O"
timeout 900 python -m pytest tests/test_gpu_hmc_shapes.py -x -q -m gpu -k "lds_prefetch or fused_stage_four or one_launch_tail" > $O/pytest1.txt 2>&1; tail -5 $O/pytest1.txt
timeout 300 python tools/timeline_r4.py > $O/tl_stash.txt 2>&1; cat $O/tl_stash.txt | tail -16
FABHIP_R4_STREAM=2 timeout 300 python tools/timeline_r4.py > $O/tl_ring.txt 2>&1; cat $O/tl_ring.txt | tail -16
timeout 600 python bench.py --full > $O/bench.json 2> $O/bench.err; python - "$O/bench.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['roofline']['frac'], d['roofline']['ms_per_launch'])
PY
FABHIP_R4_STREAM=2 timeout 600 python bench.py --full > $O/bench_ring.json 2>> $O/bench.err; python - "$O/bench_ring.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['roofline']['frac'], d['roofline']['ms_per_launch'])
PY
