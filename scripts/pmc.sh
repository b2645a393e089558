#!/bin/bash
# usage (GPU box, repo root): bash scripts/pmc.sh <tag> [bench args...]  -> ${OUT:-bench_out}/pmc_<tag>/
# Separate PMC passes (FETCH_SIZE needs 3 TCC slots, WRITE_SIZE 2: cannot share a pass), kernel-trace only.
tag=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
out=$(mkdir -p "${OUT:-$R/bench_out}" && cd "${OUT:-$R/bench_out}" && pwd)/pmc_$tag
cd /tmp && export TMPDIR=/tmp
mkdir -p $out
for ctr in FETCH_SIZE WRITE_SIZE "TCC_HIT_sum TCC_MISS_sum" "TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_32B_sum"; do
  name=$(echo $ctr | tr ' ' '_')
  rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $out/$name -o p -- python3 $R/bench.py --full --no-cpu-baseline --hbm-leg off --epoch-leg off --steps 20 --warmup 5 "$@" > $out/$name.log 2>&1 || echo "pass $name failed"
done
python3 $R/scripts/pmc_summary.py $out > $out/summary.json
cat $out/summary.json
