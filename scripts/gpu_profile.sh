# rocprofv3 kernel trace + stats of the default bench command
# usage (from the repository root): bash scripts/gpu_profile.sh OUTPUT_DIR
set -x
O=$(realpath -m "${1:?usage: bash scripts/gpu_profile.sh OUTPUT_DIR}")
R=$PWD
mkdir -p "$O"
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d "$O" -o bench -- python $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-op-leg > "$O/bench_stdout.log" 2>&1
ls -R "$O" | head -30
