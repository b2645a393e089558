#!/bin/bash
# end-of-round bench lines (--full: with their roofline legs) for every BASELINE config that fits one GPU (GPU box, repo root)
# -> ${OUT:-bench_out}/final/
out=${OUT:-bench_out}/final
mkdir -p $out
python bench.py --full --workload amazon-book --no-cpu-baseline > $out/amazon.json 2> $out/amazon.err
python bench.py --full --workload synth-1M --steps 60 --warmup 10 --no-cpu-baseline > $out/synth1m.json 2> $out/synth1m.err
python bench.py --full --workload amazon-book --model SimGCL --batch 2048 --steps 400 --warmup 40 --no-cpu-baseline > $out/simgcl_amazon.json 2> $out/simgcl_amazon.err
python bench.py --full --model MFBPR --batch 2048 --no-cpu-baseline > $out/mfbpr.json 2> $out/mfbpr.err
python bench.py --full --workload synth-10M --dim 256 --steps 15 --warmup 4 --no-cpu-baseline > $out/c5.json 2> $out/c5.err
python - $out <<'PY'
import glob, json, os, sys
for f in sorted(glob.glob(os.path.join(sys.argv[1], "*.json"))):
    for l in open(f):
        if l.startswith("{"):
            j = json.loads(l)
            print("%-16s %9.4f ms/step %12.0f %s  dense %.1f us" % (os.path.basename(f)[:-5], j["ms_per_step"], j["value"], j["unit"], (j.get("roofline") or {}).get("us_per_launch") or 0))
PY
