# Dev tool: the measurements committed under profiles/ in one gpurun call (bench line, rocprofv3 kernel stats of the same
# command, secondary configs / resample kernels, then the GPU suite).  Usage (GPU box): bash tools/final_run.sh OUT_DIR
set -x
cd ${GRAFT_REPO_ROOT:-.}
O=${1:?usage: bash tools/final_run.sh OUT_DIR}; mkdir -p "$O"
python bench.py --full 2>/dev/null | tail -1 > $O/bench.json
export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -- python bench.py --full --no-cpu-baseline --steps 20 --warmup 5 > $O/bench_prof.log 2>&1
find $O/prof -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/kernel_stats.csv
rm -rf $O/prof
python tools/bench_extra.py > $O/bench_extra.json 2> $O/bench_extra.err
python tools/bench_multinomial.py > $O/bench_multinomial.json 2>/dev/null

# spline flow (cfg 3 / cfg 5 shapes): AIS rates, stage timeline of the 8-chain kernel, per-kernel times, stream micro-benchmark
python tools/bench_spline.py 2>/dev/null | tail -1 > $O/spline_cfg3.json
FABHIP_SPLINE_MFMA=16 python tools/bench_spline.py 2>/dev/null | tail -1 > $O/spline_cfg3_16x16x4.json
CFG=5 N=3 python tools/bench_spline.py 2>/dev/null | tail -1 > $O/spline_cfg5_shape.json
python tools/timeline_spline.py 2>/dev/null | tail -14 > $O/spline_r8_stage_timeline.txt
FABHIP_TILE=16 python tools/timeline_spline.py 2>/dev/null | tail -14 > $O/spline_r8_16chain_stage_timeline.txt
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_sp -- python tools/bench_spline.py > $O/spline_prof.log 2>&1
find $O/prof_sp -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/spline_cfg3_kernel_stats.csv
rm -rf $O/prof_sp
[ -x tools/ubench/bin/nsplit ] && tools/ubench/bin/nsplit > $O/ubench_nsplit.txt 2>&1
python tools/time_hmc_shapes.py 2>/dev/null | grep "W=" > $O/hmc_tile_shapes.txt
python tools/timeline_r8.py 2048 2>/dev/null | tail -13 > $O/hmc_r8_stage_timeline.txt
python bench.py --workload cfg4 --full --no-cpu-baseline --steps 10 --warmup 3 2>/dev/null | tail -1 > $O/bench_cfg4_1gpu.json
FABHIP_BENCH_BACKEND=gloo python bench.py --gpus 2 --steps 10 --warmup 3 --full --no-cpu-baseline 2>/dev/null | tail -1 > $O/bench_2ranks_one_gpu_gloo.json
python -m pytest tests -m gpu -q -x 2>&1 | tail -4
