#!/bin/bash
# usage (on the GPU box, from the repo root): bash scripts/prof.sh <tag> [bench args...]
# kernel-trace + stats only (no PMC here; PMC passes are separate runs) of bench.py --full -> ${OUT:-bench_out}/prof_<tag>/
tag=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
out=$(mkdir -p "${OUT:-$R/bench_out}" && cd "${OUT:-$R/bench_out}" && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_$tag -o $tag -- python3 $R/bench.py --full --no-cpu-baseline --hbm-leg off --epoch-leg off "$@" > $out/prof_$tag.log 2>&1
