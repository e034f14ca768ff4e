cd $GRAFT_REPO_ROOT
O=${1:?usage: bash tools/experiments/r4f_run3.sh OUT_DIR}; mkdir -p "$O"
timeout 900 python -m pytest tests/test_gpu_fast_mode.py tests/test_gpu_hmc_shapes.py -x -q 2>&1 | tail -12 | tee $O/pytest_fast.txt
timeout 600 python bench.py --full --no-cpu-baseline > $O/bench_fast.json 2> $O/bench_fast.err; tail -3 $O/bench_fast.err
python - "$O/bench_fast.json" <<'PY'
import json, sys
for ln in open(sys.argv[1]):
    if ln.startswith('{'):
        d=json.loads(ln); print('value',d['value'],'fast',d['fast_mode']['value'],d['fast_mode']['speedup_vs_value'],d['fast_mode']['ess_trained'])
PY
