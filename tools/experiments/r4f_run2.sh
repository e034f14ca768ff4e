cd $GRAFT_REPO_ROOT
O=${1:?usage: bash tools/experiments/r4f_run2.sh OUT_DIR}; mkdir -p "$O"
timeout 1500 python -m pytest tests -m gpu -x -q 2>&1 | tail -15 | tee $O/pytest_full.txt
timeout 300 python tools/time_hmc.py 1024 2>&1 | tail -1 | tee $O/time.txt
FABHIP_R4_STREAM=1 timeout 300 python tools/time_hmc.py 1024 2>&1 | tail -1 | tee -a $O/time.txt
timeout 300 python tools/timeline_r4.py 1024 2>&1 | tail -10 | tee $O/timeline.txt
timeout 600 python bench.py --full --no-cpu-baseline > $O/bench.json 2> $O/bench.err; tail -c 1500 $O/bench.json; tail -3 $O/bench.err
