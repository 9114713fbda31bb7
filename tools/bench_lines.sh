#!/bin/bash
# The round's contract lines (configs 2 / 4 / 5 + the two extra replay schedules), run AFTER tools/collect_all.sh has put the
# round's counters into profiles/counters.json, so that every line carries its roofline (and, --full, every auxiliary leg).
#   OUT=<folder> bash tools/bench_lines.sh r04
R=${1:-r05}
OUT=${OUT:?set OUT to the folder the contract lines go to}
cd $GRAFT_REPO_ROOT
mkdir -p "$OUT"
python bench.py --full --steps 20 --warmup 5 > $OUT/${R}_bench.json 2> $OUT/${R}_bench.err
python bench.py --full --config 4 --steps 10 --warmup 2 > $OUT/${R}_bench_config4.json 2>> $OUT/${R}_bench.err
python bench.py --full --config 5 --steps 10 --warmup 2 > $OUT/${R}_bench_config5.json 2>> $OUT/${R}_bench.err
python bench.py --full --config 5 --steps 10 --warmup 2 --visibility 100,100,10,500 > $OUT/${R}_bench_config5_generalised.json 2>> $OUT/${R}_bench.err
python bench.py --full --config 5 --steps 10 --warmup 2 --visibility static > $OUT/${R}_bench_config5_static.json 2>> $OUT/${R}_bench.err
timeout 1500 python bench_configs.py > $OUT/${R}_bench_configs.jsonl 2>> $OUT/${R}_bench.err
tail -c 200 $OUT/${R}_bench.json
