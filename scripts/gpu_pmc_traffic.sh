# HBM traffic counters of the default bench command (separate --pmc passes, kernel trace only)
# usage (from the repository root): bash scripts/gpu_pmc_traffic.sh OUTPUT_DIR
set -x
O=$(realpath -m "${1:?usage: bash scripts/gpu_pmc_traffic.sh OUTPUT_DIR}")
R=$PWD
mkdir -p "$O"
cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $c -d "$O" -o $c --output-format csv -- python $R/bench.py --full --steps 3 --warmup 2 --no-cpu-baseline --no-op-timing --no-op-leg > /dev/null 2>&1
done
rocprofv3 --kernel-trace --pmc TCC_HIT_sum TCC_MISS_sum -d "$O" -o L2HIT --output-format csv -- python $R/bench.py --full --steps 3 --warmup 2 --no-cpu-baseline --no-op-timing --no-op-leg > /dev/null 2>&1
ls "$O"
