#!/bin/bash
# whole GPU suite + smoke + the default bench with every leg (--full), outputs under ${OUT:-bench_out}/all/
out=${OUT:-bench_out}/all
mkdir -p $out
timeout 2400 python -m pytest tests -x -q -m gpu > $out/pytest.txt 2>&1; echo "pytest rc=$?" >> $out/pytest.txt
python __graft_entry__.py --smoke > $out/smoke.txt 2>&1; echo "smoke rc=$?" >> $out/smoke.txt
python bench.py --full > $out/bench.json 2> $out/bench.err
for i in 1 2; do bash scripts/sharded1.sh --steps 300 --warmup 30 > $out/shard_$i.json 2> $out/shard_$i.err; done
grep -v "RCCL\|HIP version\|ROCm version\|Hostname\|Librccl" $out/pytest.txt | tail -5; tail -2 $out/smoke.txt
